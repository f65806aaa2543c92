"""Scores of the page pipeline: what did ``TextEraser`` do to a page, measured against the same page cleaned by hand?

The reference's training data are pairs of a raw page and the page cleaned by hand; its ``Dataloader.py:213-222`` derives the text mask
from such a pair (the difference of the two ``L`` images, a threshold, a 10 x 10 dilation).  ``pair_text_mask`` is that derivation on the
device, ``score_page`` compares an eraser's page and mask with the pair -- the confusion counts of the mask, the error over what was
filled, over what was left, and per text region -- and ``EraserMetrics`` / ``evaluate_eraser`` run a ``TextEraser`` over pairs and say,
per route (``flat``, ``smooth``, ``tone``, the net), how well the regions it took were repaired.  The two kernels of ``csrc/score.hip``
(semantics: ``include/tsii_hip.h``, "K18: page scores") work in integers: the same pages give the same numbers on every run.
``EraserMetrics.update()`` enqueues kernels and reads nothing back itself; the host synchronises once, in ``compute()``.  No CPU path.
"""
import math

import numpy as np
import torch

from . import _lib, ops
from ._lib import call, ptr
from .metrics import _ratio, _ssim
from .regions import _like

ROUTES = ("flat", "smooth", "tone", "net")           # who filled a region: the first three stages of TextEraser, or the filler
PAGE_WORDS = 12                                      # tp fp fn tn | fill: pixels, sum a, sum s, max m | leftover: the same four


# ---- thin wrappers of the tsii_* entry points (device tensors in, device tensors out, nothing read back) ----------------------------
def _check_page(name, t, like=None):
    if t.dim() != 3 or t.shape[2] != 3 or t.dtype != torch.uint8 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{name} must be [H, W, 3] uint8, got {tuple(t.shape)} {t.dtype}")
    if like is not None and t.shape != like.shape:
        raise ValueError(f"{name} is {tuple(t.shape)}, the other page {tuple(like.shape)}")


def _check_plane(name, t, page, dtype=torch.uint8):
    if t.dtype != dtype or tuple(t.shape) != tuple(page.shape[:2]):
        raise ValueError(f"{name} must be {list(page.shape[:2])} {dtype}, got {tuple(t.shape)} {t.dtype}")


def _on_device(*ts):
    _lib.check_device(ts[0].new_empty(0, dtype=torch.float32))          # no CPU path: host tensors are refused here
    if not all(t is None or (t.device == ts[0].device and t.is_contiguous()) for t in ts):
        raise ValueError("the pages, planes and tables of one call must be contiguous and on one device")


def _pair_text_mask(raw, clean, thr, k):
    """raw, clean uint8 [H, W, 3] -> truth uint8 [H, W] of 0 / 255 (``tsii_pair_text_mask``)"""
    h, w = int(raw.shape[0]), int(raw.shape[1])
    truth = torch.empty((h, w), dtype=torch.uint8, device=raw.device)
    _on_device(raw, clean, truth)
    call("tsii_pair_text_mask", ptr(raw), ptr(clean), h, w, int(thr), int(k), ptr(truth), _lib.stream())
    return truth


def _page_scores(out, clean, mask, truth, labels=None, table=None):
    """-> (page int64 [12], rows int64 [n, 4]) on the device (``tsii_page_scores``); ``table``: int32 [n, 6] on the device, or None"""
    h, w = int(out.shape[0]), int(out.shape[1])
    n = 0 if (labels is None or table is None) else int(table.shape[0])
    page = torch.empty((PAGE_WORDS,), dtype=torch.int64, device=out.device)
    rows = torch.empty((n, 4), dtype=torch.int64, device=out.device)
    _on_device(out, clean, mask, truth, labels, table, page, rows)
    nbytes = _lib.lib().tsii_page_scores_ws_bytes(h, w, n)
    if nbytes == 0:
        raise ValueError(f"a page of {h} x {w} pixels cannot be scored (h * w <= 2^31 - 2)")
    ws = ops._ws(nbytes, out)
    call("tsii_page_scores", ptr(out), ptr(clean), ptr(mask), ptr(truth), ptr(labels) if n else None, ptr(table) if n else None, n, h, w,
         ptr(page), ptr(rows) if n else None, ptr(ws), nbytes, _lib.stream())
    return page, rows


def _threshold(brightness_difference):
    """the integer ``thr`` with ``d > thr`` iff ``d > brightness_difference * 255`` for every integer ``d``"""
    if not 0.0 <= float(brightness_difference) <= 1.0:
        raise ValueError(f"brightness_difference {brightness_difference} must lie in [0, 1]")
    return int(math.floor(float(brightness_difference) * 255))


def _check_dilate(dilate):
    if int(dilate) != dilate or not 1 <= dilate <= 31:
        raise ValueError(f"dilate {dilate} must be an integer 1..31")
    return int(dilate)


def _to(t, dev):
    t = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t
    return t.to(dev).contiguous()


def _device_of(first, device):
    if device is not None:
        return torch.device(device)
    return first.device if (isinstance(first, torch.Tensor) and first.is_cuda) else torch.device("cuda:0")


# ---- the two functions --------------------------------------------------------------------------------------------------------------
def pair_text_mask(raw_u8, clean_u8, brightness_difference=0.4, dilate=10, device=None):
    """The text mask of a (raw page, hand-cleaned page) pair as the reference's ``Dataloader.py:213-222`` derives it: both pages to ``L``
    as Pillow converts them, ``|difference| > brightness_difference * 255``, grown by a ``dilate x dilate`` square as ``cv2.dilate``
    grows it (10: offsets -5..+4).  ``[H, W, 3]`` uint8 pages, numpy or torch, host or device -> ``[H, W]`` uint8 of 0 / 255, the same
    kind and on the same device as ``raw_u8``.  Computed on ``device`` (default: the pages', else ``cuda:0``)."""
    thr, k = _threshold(brightness_difference), _check_dilate(dilate)
    dev = _device_of(raw_u8, device)
    raw, clean = _to(raw_u8, dev), _to(clean_u8, dev)
    _check_page("raw", raw)
    _check_page("clean", clean, raw)
    return _like(_pair_text_mask(raw, clean, thr, k), raw_u8)


def score_page(out_u8, clean_u8, mask_u8, truth_u8, labels=None, table=None, device=None):
    """An eraser's page ``out_u8`` and mask ``mask_u8`` (non-zero = text) against the hand-cleaned page ``clean_u8`` and the mask
    ``truth_u8`` of the pair.  With ``d`` the absolute difference of ``out_u8`` and ``clean_u8`` per channel, ``a`` its sum over the
    channels, ``s`` the sum of its squares and ``m`` its maximum, returns a dict of numpy int64 arrays:

    ``page`` ``[12]``: ``tp, fp, fn, tn`` of the mask against the truth; ``pixels, sum a, sum s, max m`` over the pixels of the mask (the
    fill); the same four over the others (the leftover: what the mask missed);
    ``rows`` ``[n, 4]``: ``pixels, sum a, sum s, max m`` over the pixels whose label (``labels``: int32 ``[H, W]``) is ``table[r][0]``
    (``table``: int ``[n, 6]`` as ``text_regions`` returns it, ascending in its first column).  Without labels or table: ``[0, 4]``.

    numpy or torch, host or device; one synchronisation (the read-back of the two arrays)."""
    dev = _device_of(out_u8, device)
    out, clean, mask, truth = (_to(t, dev) for t in (out_u8, clean_u8, mask_u8, truth_u8))
    _check_page("out", out)
    _check_page("clean", clean, out)
    _check_plane("mask", mask, out)
    _check_plane("truth", truth, out)
    if (labels is None) != (table is None):
        raise ValueError("labels and table come together")
    if labels is not None:
        labels = _to(labels, dev)
        _check_plane("labels", labels, out, torch.int32)
        table = _table_on(table, dev)
    page, rows = _page_scores(out, clean, mask, truth, labels, table)
    both = torch.cat([page, rows.reshape(-1)]).cpu().numpy()              # the one synchronisation
    return {"page": both[:PAGE_WORDS].copy(), "rows": both[PAGE_WORDS:].reshape(-1, 4).copy()}


def _table_on(table, dev):
    """a region table as int32 ``[n, 6]`` on ``dev``.  A host table goes through pinned memory with a non-blocking copy: a copy from
    pageable memory would make the host wait for everything enqueued before it (the caching host allocator keeps the pinned block until
    the copy has run)."""
    t = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)) if not isinstance(table, torch.Tensor) else table.to(torch.int32)
    if t.dim() != 2 or t.shape[1] != 6:
        raise ValueError(f"table must be [n, 6], got {tuple(t.shape)}")
    dev = torch.device(dev)
    if dev.type == "cuda" and not t.is_cuda and t.numel():
        return t.contiguous().pin_memory().to(dev, non_blocking=True)
    return t.to(dev).contiguous()


# ---- the eraser's score ---------------------------------------------------------------------------------------------------------------
def _psnr(s, elements):
    """10 log10(255^2 / (s / elements)) in float64: inf for an error of zero, nan over no element (as ``InpaintingMetrics`` has it)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(255.0 ** 2 / _ratio(s, elements))


def _errors(pixels, a, s, m=None):
    res = {"pixels": int(pixels), "l1": float(_ratio(a, 3 * 255 * pixels)), "psnr": float(_psnr(s, 3 * pixels))}
    if m is not None:
        res["max"] = int(m)
    return res


class EraserMetrics:
    """Scores of a ``TextEraser`` over (raw page, hand-cleaned page) pairs.

    ``update(eraser, raw, clean)`` runs ``eraser(raw)`` with the page on the eraser's device, derives the truth mask from the pair
    (``pair_text_mask(raw, clean, brightness_difference, truth_dilate)``) and scores the eraser's page and mask against it
    (``score_page``), per region of the labelling the routes worked on: ``last_route_labels`` and the routes' table where ``flat``,
    ``smooth`` or ``tone`` is enabled, else ``last_labels`` and ``last_regions["table"]`` where the regions path is on, else none.  The
    route of a table row is the stage whose ``last_regions[stage]["is_*"]`` claims it, ``net`` without one.  The page's sums stay on the
    device; ``update`` reads nothing back and does not wait for the stream itself (the eraser's own synchronisation per page is the
    eraser's; the region table goes up through pinned memory without blocking; a pair given on the host is uploaded first, as the eraser
    uploads its page).

    ``compute()`` (the one device-to-host copy) returns a dict: ``mask``: ``tp, fp, fn, tn`` summed over the pages and ``precision``,
    ``recall``, ``f1``, ``iou`` (``nan`` for 0 / 0); ``fill`` and ``leftover``: ``pixels``, ``l1`` (the mean absolute error per channel
    over 255), ``psnr`` (dB at a peak of 255; ``inf`` for an error of zero, ``nan`` over no pixel) and ``max`` (grey levels) over the pixels
    of the eraser's mask and over the others (where the eraser returns the page: the ink its mask missed); ``routes``: per route
    ``regions``, ``pixels``, ``l1``, ``psnr`` and ``worst``: the region with the largest mean error, as ``{"l1", "page", "row"}`` (the index
    of the update and the table row; ``None`` without a region); ``pages``: per update ``{"page", "rows", "route", "table"}``, the arrays of
    ``score_page``, the index into ``ROUTES`` of every row and the table the rows belong to (``"ssim"`` too with ``ssim=True``: the SSIM
    of the eraser's page against the hand-cleaned one, whose mean over the pages is ``ssim`` at the top; pages of at least 11 x 11)."""

    def __init__(self, brightness_difference=0.4, truth_dilate=10, ssim=False):
        self.thr, self.k, self.ssim = _threshold(brightness_difference), _check_dilate(truth_dilate), bool(ssim)
        self._pages = []                                 # per update: (page int64 [12], rows int64 [n, 4], ssim double [1] or None) on the device, route int8 [n], table

    def reset(self):
        self._pages = []

    def update(self, eraser, raw, clean):
        raw_d, clean_d = eraser._upload(raw), eraser._upload(clean)
        _check_page("clean", clean_d, raw_d)
        out, mask = eraser(raw_d)
        truth = _pair_text_mask(raw_d, clean_d, self.thr, self.k)
        labels, table = None, None
        regions = eraser.last_regions if eraser.regions else None
        stages = [name for name in ROUTES[:3] if regions is not None and name in regions]
        if stages:
            labels, table = eraser.last_route_labels, regions[stages[0]]["table"]
        elif regions is not None:
            labels, table = eraser.last_labels, regions["table"]
        table = np.zeros((0, 6), np.int32) if table is None else table
        route = np.full(len(table), ROUTES.index("net"), np.int8)
        for name in reversed(stages):                    # a region belongs to the first stage that took it
            route[regions[name]["is_" + name]] = ROUTES.index(name)
        page, rows = _page_scores(out, clean_d, mask, truth, labels, _table_on(table, out.device) if len(table) else None)
        ssim = _ssim(out.unsqueeze(0).float(), clean_d.unsqueeze(0).float(), 255.0) if self.ssim else None
        self._pages.append((page, rows, ssim, route, table))

    def compute(self):
        words = [t.reshape(-1) for page, rows, _, _, _ in self._pages for t in (page, rows)]
        words += [ssim.view(torch.int64) for _, _, ssim, _, _ in self._pages if ssim is not None]
        host = torch.cat(words).cpu().numpy() if words else np.zeros(0, np.int64)        # the one synchronisation
        pages, at = [], 0
        for _, rows, _, route, table in self._pages:
            n = int(rows.shape[0])
            pages.append({"page": host[at:at + PAGE_WORDS].copy(), "rows": host[at + PAGE_WORDS:at + PAGE_WORDS + 4 * n].reshape(n, 4).copy(),
                          "route": route, "table": table})
            at += PAGE_WORDS + 4 * n
        if self.ssim:
            for p, v in zip(pages, host[at:].view(np.float64)):
                p["ssim"] = float(v)
        total = np.sum([p["page"] for p in pages], axis=0, dtype=np.int64) if pages else np.zeros(PAGE_WORDS, np.int64)
        tp, fp, fn, tn = (int(v) for v in total[:4])
        res = {"mask": {"tp": tp, "fp": fp, "fn": fn, "tn": tn, "precision": float(_ratio(tp, tp + fp)), "recall": float(_ratio(tp, tp + fn)),
                        "f1": float(_ratio(2 * tp, 2 * tp + fp + fn)), "iou": float(_ratio(tp, tp + fp + fn))}}
        for name, at in (("fill", 4), ("leftover", 8)):
            res[name] = _errors(total[at], total[at + 1], total[at + 2], max([int(p["page"][at + 3]) for p in pages], default=0))
        res["routes"] = {}
        for code, name in enumerate(ROUTES):
            sums, regions, worst = np.zeros(3, np.int64), 0, None
            for i, p in enumerate(pages):
                mine = p["rows"][p["route"] == code]
                regions += len(mine)
                sums += mine[:, :3].sum(axis=0, dtype=np.int64)
                mean = _ratio(p["rows"][:, 1], 3 * 255 * p["rows"][:, 0])
                mean = np.where((p["route"] == code) & ~np.isnan(mean), mean, -1.0)
                if len(mean) and mean.max() >= 0 and (worst is None or mean.max() > worst["l1"]):
                    worst = {"l1": float(mean.max()), "page": i, "row": int(mean.argmax())}
            res["routes"][name] = dict(regions=regions, **_errors(*sums), worst=worst)
        if self.ssim:
            res["ssim"] = float(np.mean([p["ssim"] for p in pages])) if pages else float("nan")
        res["pages"] = pages
        return res


def evaluate_eraser(eraser, pairs, metrics=None):
    """``pairs`` yields ``(raw_u8, clean_u8)``: a page and the same page cleaned by hand, ``[H, W, 3]`` uint8, numpy or torch.  Returns
    ``metrics.compute()`` (``EraserMetrics()`` by default; pass one to choose the truth's threshold or to keep accumulating)."""
    metrics = EraserMetrics() if metrics is None else metrics
    for raw, clean in pairs:
        metrics.update(eraser, raw, clean)
    return metrics.compute()
