"""Validation metrics on the device: is this checkpoint better than that one?

``SegmentationMetrics`` (precision / recall / F1 / IoU at up to 32 thresholds in one pass, and the threshold to hand to
``TextEraser``) and ``InpaintingMetrics`` (L1, PSNR, SSIM of the composite) sit on the three kernels of ``csrc/metrics.hip``
(semantics: ``include/tsii_hip.h``, "K9: validation metrics").  ``update()`` enqueues kernels and reads nothing back; the host
synchronises once, in ``compute()``.  ``evaluate_segmentation`` / ``evaluate_inpainting`` run a net over batches in ``eval()``
mode under ``torch.no_grad()`` and leave every ``training`` flag as they found it.  No CPU path: host tensors are refused.
"""
import ctypes

import numpy as np
import torch

from . import _lib, ops
from ._lib import call, ptr
from .BaseModels import to_nhwc
from .masks import MaskParts
from .pipeline import _eval_mode, logit_of

MAX_THRESHOLDS = 32


# ---- thin wrappers of the tsii_* entry points ---------------------------------------------------------------------------------------
def _seg_confusion(logits, target, logit_thresholds):
    """logits, target fp32 [N, H, W] -> int32 [N, 2, K + 1] (class, number of thresholds exceeded)"""
    _lib.check_device(logits, target)
    assert logits.shape == target.shape and logits.dim() == 3 and logits.is_contiguous() and target.is_contiguous()
    k = len(logit_thresholds)
    thr = (ctypes.c_float * k)(*logit_thresholds)                # host array: read during the call
    hist = torch.empty((logits.shape[0], 2, k + 1), dtype=torch.int32, device=logits.device)
    call("tsii_seg_confusion", ptr(logits), ptr(target), int(logits.shape[0]), int(logits.shape[1] * logits.shape[2]), thr, k, ptr(hist),
         _lib.stream())
    return hist


def _inpaint_errors(out, clean, mask, clamp01):
    """out, clean fp32 NHWC; mask NHWC or a plane [N, H, W] -> double [N, 5]: hole elements, sum |d| / d^2 over holes, over valid"""
    _lib.check_device(out, clean, mask)
    n, h, w, c = out.shape
    plane = mask.dim() == 3
    assert clean.shape == out.shape and tuple(mask.shape) == ((n, h, w) if plane else (n, h, w, c))
    assert out.is_contiguous() and clean.is_contiguous() and mask.is_contiguous()
    sums = torch.empty((n, 5), dtype=torch.float64, device=out.device)
    nbytes = _lib.lib().tsii_inpaint_errors_ws_bytes(n, h, w, c)
    ws = ops._ws(nbytes, out)
    call("tsii_inpaint_errors", ptr(out), ptr(clean), ptr(mask), int(plane), int(bool(clamp01)), n, h, w, c, ptr(sums), ptr(ws), nbytes,
         _lib.stream())
    return sums


def _ssim(a, b, data_range=1.0):
    """a, b fp32 NHWC [N, H, W, C <= 4], H, W >= 11 -> per-image mean SSIM, double [N]"""
    _lib.check_device(a, b)
    n, h, w, c = a.shape
    assert b.shape == a.shape and a.is_contiguous() and b.is_contiguous()
    if h < 11 or w < 11 or not 1 <= c <= 4:
        raise ValueError(f"SSIM needs images of at least 11 x 11 pixels and 1..4 channels, got {h} x {w} x {c}")
    out = torch.empty((n,), dtype=torch.float64, device=a.device)
    nbytes = _lib.lib().tsii_ssim_ws_bytes(n, h, w, c)
    ws = ops._ws(nbytes, a)
    call("tsii_ssim", ptr(a), ptr(b), n, h, w, c, float(data_range), ptr(out), ptr(ws), nbytes, _lib.stream())
    return out


def _f32(t):
    return t if t.dtype == torch.float32 else t.float()           # bf16 activation storage: cast once, here


def _ratio(num, den):
    """float64 num / den; 0 / 0 is nan (a metric that does not exist is not 0 and not 1)"""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.nan)


# ---- segmentation ------------------------------------------------------------------------------------------------------------------
class SegmentationMetrics:
    """Confusion counts of a text segmenter at several thresholds, accumulated on the device.

    ``thresholds``: text probabilities in (0, 1) (``sigmoid(logit) > p``, compared as ``logit > logit_of(p)`` in fp32 -- the very
    test ``TextEraser(threshold=p)`` applies), at most 32, kept in ascending order; an int ``n`` means ``n`` evenly spaced
    probabilities ``1 / (n + 1) .. n / (n + 1)``.  ``update(logits, target)`` takes ``[N,1,H,W]`` or ``[N,H,W]`` (fp32, or bf16
    logits); a pixel is text where ``target > 0.5``.  ``compute()`` does the one device-to-host copy and returns a dict:
    ``thresholds`` and, as lists in the same order, ``tp``, ``fp``, ``fn``, ``tn`` (ints), ``precision``, ``recall``, ``f1``,
    ``iou``, ``accuracy`` (float64, ``nan`` for 0 / 0); ``pixels``; ``best_threshold`` (highest F1, the lowest such threshold on
    ties, ``nan`` when no F1 exists).
    """

    def __init__(self, thresholds=(0.5,)):
        if isinstance(thresholds, (int, np.integer)) and not isinstance(thresholds, bool):
            n = int(thresholds)
            if not 1 <= n <= MAX_THRESHOLDS:
                raise ValueError(f"{n} thresholds: 1..{MAX_THRESHOLDS}")
            thresholds = [(i + 1) / (n + 1) for i in range(n)]
        probs = sorted(float(p) for p in thresholds)
        if not 1 <= len(probs) <= MAX_THRESHOLDS:
            raise ValueError(f"{len(probs)} thresholds: 1..{MAX_THRESHOLDS}")
        if any(not 0.0 < p < 1.0 for p in probs):
            raise ValueError("thresholds are probabilities in (0, 1)")
        self.thresholds = tuple(probs)
        self.logit_thresholds = tuple(logit_of(p) for p in probs)
        self._acc = None                                          # int64 [2, K + 1] on the device of the first update

    def reset(self):
        self._acc = None

    def update(self, logits, target):
        if logits.dim() == 4:
            if logits.shape[1] != 1:
                raise ValueError(f"logits {tuple(logits.shape)}: [N,1,H,W] or [N,H,W]")
            logits = logits.reshape(logits.shape[0], logits.shape[2], logits.shape[3])
        if target.dim() == 4:
            target = target.reshape(target.shape[0], target.shape[2], target.shape[3])
        if logits.dim() != 3 or target.shape != logits.shape:
            raise ValueError(f"logits {tuple(logits.shape)} and target {tuple(target.shape)} must be [N,1,H,W] or [N,H,W] of one size")
        _lib.check_device(logits, target, bf16_ok=True)
        hist = _seg_confusion(_f32(logits).contiguous(), _f32(target).contiguous(), self.logit_thresholds)
        s = hist.sum(dim=0, dtype=torch.int64)
        self._acc = s if self._acc is None else self._acc + s

    def compute(self):
        k = len(self.thresholds)
        h = np.zeros((2, k + 1), np.int64) if self._acc is None else self._acc.cpu().numpy()     # the one synchronisation
        above = np.cumsum(h[:, ::-1], axis=1)[:, ::-1]            # above[c, b] = pixels of class c exceeding at least b thresholds
        tp, fp = above[1, 1:], above[0, 1:]
        fn, tn = above[1, 0] - tp, above[0, 0] - fp
        pixels = int(h.sum())
        f1 = _ratio(2 * tp, 2 * tp + fp + fn)
        best = float("nan")
        if not np.all(np.isnan(f1)):
            best = self.thresholds[int(np.nanargmax(f1))]         # the first maximum: the lowest threshold on ties
        return {"thresholds": list(self.thresholds), "tp": [int(v) for v in tp], "fp": [int(v) for v in fp], "fn": [int(v) for v in fn],
                "tn": [int(v) for v in tn], "precision": _ratio(tp, tp + fp).tolist(), "recall": _ratio(tp, tp + fn).tolist(),
                "f1": f1.tolist(), "iou": _ratio(tp, tp + fp + fn).tolist(), "accuracy": _ratio(tp + tn, np.full(k, pixels)).tolist(),
                "pixels": pixels, "best_threshold": best}


# ---- inpainting --------------------------------------------------------------------------------------------------------------------
def _mask_form(mask, n, c, h, w):
    """the mask as the kernel takes it: one plane [N,H,W] where the channels share it, NHWC otherwise"""
    if isinstance(mask, MaskParts):
        if len(mask.parts) != 1 or mask.channels != c:
            raise ValueError("the mask must cover the image's channels in one part")
        p = mask.parts[0]
        mask = p.plane if p.planar else p.full
        return _f32(mask).contiguous()
    if mask.dim() == 3:
        return _f32(mask).contiguous()
    if mask.dim() != 4 or mask.shape[1] not in (1, c):
        raise ValueError(f"mask {tuple(mask.shape)}: [N,{c},H,W], [N,1,H,W], [N,H,W] or MaskParts")
    if mask.shape[1] == 1 or mask.stride(1) == 0:
        return _f32(mask[:, 0]).contiguous()
    return to_nhwc(_f32(mask))


class InpaintingMetrics:
    """L1, PSNR and SSIM of an inpainting net's output, accumulated per image on the device.

    ``update(out, clean, mask)``: ``out``, ``clean`` ``[N,C,H,W]`` (channels-last memory costs no copy), ``mask`` a ``[N,C,H,W]``
    tensor, a ``[N,H,W]`` plane or a ``MaskParts``; 1 = keep, 0 = hole.  With ``clamp`` the output is clamped to [0, 1] first,
    as ``TextEraser`` does before it writes bytes.  ``compute()`` (the one device-to-host copy) returns the mean over images of
    ``l1_hole``, ``l1_valid`` (mean |out - clean| over hole / valid elements), ``psnr`` (the output as it is), ``psnr_composite``
    (``clean`` on valid pixels: only the holes' squared error counts, over all elements), ``psnr_hole`` (holes only), each
    ``10 log10(data_range^2 / mse)`` averaged in dB, and ``ssim_composite`` (mean SSIM between ``mask * clean + (1 - mask) * out``
    and ``clean``; left out with ``ssim=False``).  An image without holes has no ``l1_hole`` and infinite ``psnr_hole`` /
    ``psnr_composite``: it is left out of those three means and counted in ``images_without_holes`` (an image that is all hole is
    left out of ``l1_valid`` likewise); a mean over no image is ``nan``.  ``images`` is the number of images seen.
    """

    def __init__(self, data_range=1.0, clamp=True, ssim=True):
        if not float(data_range) > 0:
            raise ValueError("data_range > 0")
        self.data_range, self.clamp, self.ssim = float(data_range), bool(clamp), bool(ssim)
        self._rows = []                                           # per update: double [N, 7] = 5 sums, elements per image, SSIM

    def reset(self):
        self._rows = []

    def update(self, out, clean, mask):
        if out.dim() != 4 or clean.shape != out.shape:
            raise ValueError(f"out {tuple(out.shape)} and clean {tuple(clean.shape)} must be [N,C,H,W] of one size")
        n, c, h, w = out.shape
        m = _mask_form(mask, n, c, h, w)
        _lib.check_device(out, clean, m, bf16_ok=True)
        o, g = to_nhwc(_f32(out)), to_nhwc(_f32(clean))
        sums = _inpaint_errors(o, g, m, self.clamp)
        cols = [sums, torch.full((n, 1), float(h * w * c), dtype=torch.float64, device=o.device)]
        if self.ssim:
            full = m if m.dim() == 4 else m.unsqueeze(-1).expand(-1, -1, -1, c).contiguous()
            comp = ops.compose(g, full, o.clamp(0.0, 1.0) if self.clamp else o)
            cols.append(_ssim(comp, g, self.data_range).unsqueeze(1))
        self._rows.append(torch.cat(cols, dim=1))

    def compute(self):
        width = 7 if self.ssim else 6
        r = torch.cat(self._rows, dim=0).cpu().numpy() if self._rows else np.zeros((0, width))    # the one synchronisation
        cnt, h1, h2, v1, v2, numel = (r[:, i] for i in range(6))
        peak = self.data_range ** 2

        def psnr(se, over):
            with np.errstate(divide="ignore", invalid="ignore"):
                return 10.0 * np.log10(peak / (se / over))

        def mean(v, keep=None):
            v = v if keep is None else v[keep]
            return float(np.mean(v)) if v.size else float("nan")
        holes, valid = cnt > 0, cnt < numel
        res = {"l1_hole": mean(_ratio(h1, cnt), holes), "l1_valid": mean(_ratio(v1, numel - cnt), valid),
               "psnr": mean(psnr(h2 + v2, numel)), "psnr_composite": mean(psnr(h2, numel), holes),
               "psnr_hole": mean(psnr(h2, np.where(holes, cnt, 1.0)), holes)}
        if self.ssim:
            res["ssim_composite"] = mean(r[:, 6])
        res["images_without_holes"] = int((~holes).sum())
        res["images"] = int(r.shape[0])
        return res


# ---- evaluation loops --------------------------------------------------------------------------------------------------------------
def _to_device_of(net, *tensors):
    """the batch on the net's device (a net without parameters -- a plain callable -- takes the batch where it is)"""
    p = next(net.parameters(), None) if isinstance(net, torch.nn.Module) else None
    if p is None:
        return tensors
    return tuple(t if isinstance(t, MaskParts) or t.device == p.device else t.to(p.device, non_blocking=True) for t in tensors)


def evaluate_segmentation(net, batches, metrics=None):
    """``net``: ``x[N,3,H,W] -> logits[N,1,H,W]``; ``batches`` yields ``(image, target)`` as ``TextSegmentationData`` collates them,
    on the device or to be moved there.  Returns ``metrics.compute()`` (``SegmentationMetrics()`` by default; pass one to choose
    the thresholds or to keep accumulating)."""
    metrics = SegmentationMetrics() if metrics is None else metrics
    with torch.no_grad(), _eval_mode(net):
        for image, target in batches:
            image, target = _to_device_of(net, image, target)
            metrics.update(net(image), target)
    return metrics.compute()


def evaluate_inpainting(net, batches, metrics=None):
    """``net``: called with the pair ``(corrupted, mask)`` (``ImageFill``'s convention) ``-> out[N,3,H,W]``; ``batches`` yields
    ``(corrupted, mask, clean)`` as ``ImageInpaintingData`` collates them.  Returns ``metrics.compute()``."""
    metrics = InpaintingMetrics() if metrics is None else metrics
    with torch.no_grad(), _eval_mode(net):
        for corrupted, mask, clean in batches:
            corrupted, mask, clean = _to_device_of(net, corrupted, mask, clean)
            metrics.update(net((corrupted, mask)), clean, mask)
    return metrics.compute()
