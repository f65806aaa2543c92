"""A filler that is a kernel and not a net: the harmonic fill of ``csrc/harmonic.hip`` (include/tsii_hip.h, "K14: harmonic fill").

The holes of an image are filled with the smooth continuation of the pixels around them -- Laplace's equation over the holes with the
valid pixels as the boundary, in one coarse-to-fine pass on the device: a pyramid of means of the valid pixels, then, level by level
back down, every hole starts from its relaxed parent and takes ``sweeps`` Jacobi sweeps.  It is the right fill for text on a smooth
background (a gradient, a soft shadow, a sky) and needs no inpainting checkpoint:

    eraser = T.TextEraser(T.XceptionTextSegment().cuda(), T.HarmonicFill())

``HarmonicFill`` obeys the ``filler`` calling convention of ``TextEraser``; ``harmonic_fill`` is the stand-alone form for a uint8 page
and a mask.  Device tensors only: there is no CPU path.

The same solver carries the seamless composition of ANOTHER filler's output (``csrc/blend.hip``, "K20: seamless fill"): an inpainting net
reproduces structure well and absolute level badly, and its error at the valid pixels around a hole, continued harmonically into the hole
and added there, takes the level of the patch back to that of its surroundings (Poisson cloning of the net's output into the page).
``SeamlessFill(filler)`` wraps any filler, ``seamless_fill`` is the stand-alone form for a page, somebody's fill of it and a mask, and
``TextEraser(blend=True)`` runs it between the filler and compose.

Neither of the two invents texture.  ``PatchFill`` does (``csrc/patch.hip``, "K21: patch fill"): every hole pixel becomes a COPY of a page
pixel whose neighbourhood matches the hole pixel's own -- an edge, hatching or screentone running under the text is continued with the
page's own pixels -- found by a PatchMatch-style search of a nearest-neighbour field, coarse to fine, from the harmonic fill as the
first guess.  ``patch_fill`` is the stand-alone form for a page and a mask.
"""
import numpy as np
import torch

from . import _lib, ops
from ._lib import call, ptr
from .masks import MaskParts

MAX_SWEEPS = 16                 # what tsii_harmonic_fill accepts (the LDS a block has for its patch and apron)
MAX_PATCH, MAX_LEVELS, MAX_ITERS = 9, 6, 8      # what tsii_patch_fill accepts (radius 1..4)


def check_sweeps(sweeps):
    if isinstance(sweeps, bool) or int(sweeps) != sweeps or not 0 <= sweeps <= MAX_SWEEPS:
        raise ValueError(f"sweeps {sweeps} must be an integer in 0..{MAX_SWEEPS}")
    return int(sweeps)


def _check_int(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"{name} {v!r} must be an integer in {lo}..{hi}")
    return int(v)


def check_patch_args(patch, levels, iters, seed):
    """-> (radius, levels, iters, seed) of ``tsii_patch_fill``: ``patch`` odd in 3..9, ``levels`` 1..6, ``iters`` 1..8, ``seed`` 32 bits"""
    patch = _check_int("patch", patch, 3, MAX_PATCH)
    if patch % 2 == 0:
        raise ValueError(f"patch {patch} must be odd (3, 5, 7 or 9): the window is centred on its pixel")
    return patch // 2, _check_int("levels", levels, 1, MAX_LEVELS), _check_int("iters", iters, 1, MAX_ITERS), _check_int("seed", seed, 0, 2 ** 32 - 1)


def _patch_fill(page_u8_nhwc, hole_u8, init_u8, radius, levels, iters, seed):
    """uint8 ``[n, h, w, 3]`` page, uint8 ``[n, h, w]`` hole plane (hole iff != 0) and uint8 ``[n, h, w, 3]`` first guess (read under the
    holes only) -> ``(out uint8 [n, h, w, 3], nnf int32 [n, h, w, 2], stats int32 [n, 3])`` (``tsii_patch_fill``): device tensors, nothing
    is read back; what the page holds under a hole is never used"""
    n, h, w, c = (int(v) for v in page_u8_nhwc.shape)
    assert c == 3 and tuple(hole_u8.shape) == (n, h, w) and tuple(init_u8.shape) == (n, h, w, 3)
    assert page_u8_nhwc.dtype == hole_u8.dtype == init_u8.dtype == torch.uint8
    _lib.check_device(page_u8_nhwc.new_empty(0, dtype=torch.float32))       # no CPU path: the byte planes' device goes into the check
    assert page_u8_nhwc.device == hole_u8.device == init_u8.device
    assert page_u8_nhwc.is_contiguous() and hole_u8.is_contiguous() and init_u8.is_contiguous()
    nbytes = int(_lib.lib().tsii_patch_fill_ws_bytes(n, h, w, int(radius), int(levels)))
    if nbytes == 0:
        raise ValueError(f"patch fill: {n} images of {h} x {w} pixels (every extent >= 1, fewer than 2^31 elements), radius {radius} (1..4), "
                         f"levels {levels} (1..{MAX_LEVELS})")
    out = torch.empty_like(page_u8_nhwc)
    nnf = torch.empty((n, h, w, 2), dtype=torch.int32, device=out.device)
    stats = torch.empty((n, 3), dtype=torch.int32, device=out.device)
    ws = ops._ws(nbytes, out)
    call("tsii_patch_fill", ptr(page_u8_nhwc), ptr(hole_u8), ptr(init_u8), n, h, w, int(radius), int(levels), int(iters), int(seed), ptr(out),
         ptr(nnf), ptr(stats), ptr(ws), _lib.stream())
    return out, nnf, stats


def _harmonic_fill(x_nhwc, plane, sweeps):
    """fp32 NHWC ``[n, h, w, 3]`` and its validity plane fp32 ``[n, h, w]`` (valid iff != 0) -> the filled fp32 NHWC tensor
    (``tsii_harmonic_fill``); what ``x_nhwc`` holds under a hole is never read"""
    n, h, w, c = (int(v) for v in x_nhwc.shape)
    assert c == 3 and tuple(plane.shape) == (n, h, w)
    _lib.check_device(x_nhwc, plane)
    assert x_nhwc.device == plane.device and x_nhwc.is_contiguous() and plane.is_contiguous()
    nbytes = int(_lib.lib().tsii_harmonic_fill_ws_bytes(n, h, w))
    if nbytes == 0:
        raise ValueError(f"harmonic fill: {n} images of {h} x {w} pixels (every extent >= 1, at most 2^31 elements)")
    out = torch.empty_like(x_nhwc)
    ws = ops._ws(nbytes, x_nhwc)
    call("tsii_harmonic_fill", ptr(x_nhwc), ptr(plane), n, h, w, int(sweeps), ptr(out), ptr(ws), _lib.stream())
    return out


def _seamless_fill(x_nhwc, out_nhwc, plane, sweeps):
    """fp32 NHWC ``[n, h, w, 3]`` twice -- the image as the filler saw it and the filler's output -- and the validity plane fp32
    ``[n, h, w]`` (valid iff != 0) -> the blended output, a new fp32 NHWC tensor (``tsii_seamless_fill``): ``out_nhwc`` bit for bit on the
    valid pixels, its clamped value plus the harmonic continuation of ``x - clamp(out)`` under the holes; what ``x_nhwc`` holds under a
    hole is never read"""
    n, h, w, c = (int(v) for v in x_nhwc.shape)
    assert c == 3 and tuple(out_nhwc.shape) == (n, h, w, 3) and tuple(plane.shape) == (n, h, w)
    _lib.check_device(x_nhwc, out_nhwc, plane)
    assert x_nhwc.device == out_nhwc.device == plane.device and x_nhwc.is_contiguous() and out_nhwc.is_contiguous() and plane.is_contiguous()
    nbytes = int(_lib.lib().tsii_seamless_fill_ws_bytes(n, h, w))
    if nbytes == 0:
        raise ValueError(f"seamless fill: {n} images of {h} x {w} pixels (every extent >= 1, at most 2^31 elements)")
    dst = torch.empty_like(out_nhwc)
    ws = ops._ws(nbytes, x_nhwc)
    call("tsii_seamless_fill", ptr(x_nhwc), ptr(out_nhwc), ptr(plane), n, h, w, int(sweeps), ptr(dst), ptr(ws), _lib.stream())
    return dst


def _validity_plane(mask, n, h, w):
    """one fp32 plane ``[n, h, w]`` from a ``MaskParts`` of one planar part, a tensor ``[N,1,H,W]`` / ``[N,3,H,W]`` with equal
    channels, or a plane ``[N,H,W]``"""
    if isinstance(mask, torch.Tensor) and mask.dim() == 3:
        plane = mask
    else:
        if isinstance(mask, torch.Tensor):
            if mask.dim() != 4 or mask.shape[1] not in (1, 3):
                raise ValueError(f"mask must be [N,1,H,W], [N,3,H,W] with equal channels or [N,H,W], got {tuple(mask.shape)}")
            mask = MaskParts.from_tensor(mask)
        if not isinstance(mask, MaskParts) or len(mask.parts) != 1:
            raise ValueError("mask must be a MaskParts of one part, a tensor [N,1,H,W] / [N,3,H,W] or a plane [N,H,W]")
        part = mask.parts[0]
        if part.planar:
            plane = part.plane
        else:                                           # a materialised [N,H,W,C] mask: one plane only if its channels agree
            full = part.full
            if not bool((full == full[..., :1]).all()):
                raise ValueError("harmonic fill: the 3 channels share one validity plane; a per-channel mask is refused")
            plane = full[..., 0]
    if tuple(plane.shape) != (n, h, w):
        raise ValueError(f"mask plane {tuple(plane.shape)} for {n} images of {h} x {w}")
    return plane.float().contiguous()


class HarmonicFill:
    """``out[N,3,H,W] = HarmonicFill(sweeps=8)((x[N,3,H,W], mask))``: the ``filler`` of a ``TextEraser`` without a net.  ``mask`` is 1
    (non-zero) where ``x`` is valid and 0 over the holes: a ``MaskParts`` of one planar part (what ``TextEraser`` passes), a tensor
    ``[N,1,H,W]`` or ``[N,3,H,W]`` with equal channels, or a plane ``[N,H,W]``.  A channels-last ``x`` is used without a copy; the
    result is the NCHW-shaped view of the NHWC output.  Valid pixels come back bit for bit; what ``x`` holds under a hole is never
    read.  ``sweeps`` (0..16) Jacobi sweeps per level: 8 puts interior holes of a smooth page within one grey level of the exact
    harmonic solution.  Not an ``nn.Module``: no parameters, nothing to load."""

    def __init__(self, sweeps=8):
        self.sweeps = check_sweeps(sweeps)

    def __call__(self, args):
        x, mask = args
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"x must be [N,3,H,W], got {tuple(getattr(x, 'shape', ()))}")
        n, _, h, w = (int(v) for v in x.shape)
        plane = _validity_plane(mask, n, h, w)
        out = _harmonic_fill(x.float().permute(0, 2, 3, 1).contiguous(), plane, self.sweeps)
        return out.permute(0, 3, 1, 2)

    def __repr__(self):
        return f"HarmonicFill(sweeps={self.sweeps})"


def _quantise(t):
    """fp32 in [0, 1] -> uint8, the compose kernels' rounding"""
    return torch.floor(t.clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8)


class PatchFill:
    """``out[N,3,H,W] = PatchFill(patch=7, levels=4, iters=4, seed=0, sweeps=8)((x[N,3,H,W], mask))``: the ``filler`` of a ``TextEraser``
    that continues what runs UNDER the text -- a panel border, an outline, hatching, screentone of any pitch -- with the page's own
    pixels and without a net.  ``x`` is ``page / 255 * mask`` as ``TextEraser`` passes it (any fp32 in [0, 1] works: it is quantised with
    ``floor(clamp(x, 0, 1) * 255 + 0.5)``), ``mask`` as for ``HarmonicFill``.  The first guess is ``HarmonicFill(sweeps)`` of the same pair;
    ``tsii_patch_fill`` then searches, coarse to fine over ``levels`` levels and ``iters`` iterations each, for every hole pixel the
    pixel of the same image whose ``patch x patch`` window (odd, 3..9; free of holes) matches the hole pixel's own best, and copies it.
    Every output pixel under a hole is therefore a pixel ``x`` holds somewhere else (the harmonic value where an image has no window
    without a hole); valid pixels come back as ``x`` quantised, which for a uint8 page over 255 is ``x`` bit for bit.  All integer: the
    same bits on every run; another ``seed`` (32 bits) gives another, equally good, fill.  No synchronisation; the result is the
    NCHW-shaped view of an NHWC tensor.  Not an ``nn.Module``: no parameters, nothing to load."""

    def __init__(self, patch=7, levels=4, iters=4, seed=0, sweeps=8):
        self.radius, self.levels, self.iters, self.seed = check_patch_args(patch, levels, iters, seed)
        self.patch, self.sweeps = 2 * self.radius + 1, check_sweeps(sweeps)

    def __call__(self, args):
        x, mask = args
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"x must be [N,3,H,W], got {tuple(getattr(x, 'shape', ()))}")
        n, _, h, w = (int(v) for v in x.shape)
        plane = _validity_plane(mask, n, h, w)
        x_nhwc = x.float().permute(0, 2, 3, 1).contiguous()
        init = _harmonic_fill(x_nhwc, plane, self.sweeps)
        hole = (plane == 0).to(torch.uint8)
        out, _, _ = _patch_fill(_quantise(x_nhwc), hole, _quantise(init), self.radius, self.levels, self.iters, self.seed)
        return (out.float() / 255.0).permute(0, 3, 1, 2)

    def __repr__(self):
        return f"PatchFill(patch={self.patch}, levels={self.levels}, iters={self.iters}, seed={self.seed}, sweeps={self.sweeps})"


class SeamlessFill:
    """``out[N,3,H,W] = SeamlessFill(filler, sweeps=8)((x[N,3,H,W], mask))``: ``filler`` -- anything that obeys the ``filler`` calling
    convention of ``TextEraser`` -- with its output taken into ``x`` in the gradient domain (``tsii_seamless_fill``, "K20: seamless fill").
    The inner filler is called with the same pair; where ``mask`` is 1 (non-zero) its output comes back bit for bit, over the holes its
    output clamped to [0, 1] plus the harmonic continuation (``sweeps`` 0..16, as ``HarmonicFill``) of its own error ``x - clamp(out)`` on
    the valid pixels: the gradients of the filler, the level of the surroundings.  ``mask`` in the forms ``HarmonicFill`` accepts; what
    ``x`` holds under a hole reaches the inner filler only.  The result is the NCHW-shaped view of an NHWC tensor.
    ``TextEraser(segmenter, filler, blend=True)`` is ``TextEraser(segmenter, SeamlessFill(filler))`` without the wrapper."""

    def __init__(self, filler, sweeps=8):
        if not callable(filler):
            raise TypeError("filler must be callable: (x[N,3,H,W], mask) -> out[N,3,H,W]")
        self.filler, self.sweeps = filler, check_sweeps(sweeps)

    def __call__(self, args):
        x, mask = args
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"x must be [N,3,H,W], got {tuple(getattr(x, 'shape', ()))}")
        n, _, h, w = (int(v) for v in x.shape)
        plane = _validity_plane(mask, n, h, w)
        out = self.filler((x, mask))
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != (n, 3, h, w):
            raise ValueError(f"filler returned {tuple(getattr(out, 'shape', ()))} for x {tuple(x.shape)}")
        nhwc = lambda t: t.float().permute(0, 2, 3, 1).contiguous()
        return _seamless_fill(nhwc(x), nhwc(out), plane, self.sweeps).permute(0, 3, 1, 2)

    def __repr__(self):
        return f"SeamlessFill({self.filler!r}, sweeps={self.sweeps})"


def _page_and_plane(page_u8, mask_u8, what="page"):
    p = torch.from_numpy(np.ascontiguousarray(page_u8)) if isinstance(page_u8, np.ndarray) else page_u8
    m = torch.from_numpy(np.ascontiguousarray(mask_u8)) if isinstance(mask_u8, np.ndarray) else mask_u8
    if not isinstance(p, torch.Tensor) or p.dim() != 3 or p.shape[2] != 3 or p.dtype != torch.uint8 or p.shape[0] < 1 or p.shape[1] < 1:
        raise ValueError(f"{what} must be [H, W, 3] uint8, got {tuple(getattr(p, 'shape', ()))} {getattr(p, 'dtype', type(p))}")
    if not isinstance(m, torch.Tensor) or m.dtype != torch.uint8 or tuple(m.shape) != tuple(p.shape[:2]):
        raise ValueError(f"mask must be [H, W] uint8 for a page of {tuple(p.shape)}, got {tuple(getattr(m, 'shape', ()))} "
                         f"{getattr(m, 'dtype', type(m))}")
    return p, m


def seamless_fill(page_u8, fill_u8, mask_u8, sweeps=8, device=None):
    """``clean_u8``: ``page_u8`` with the pixels under the mask taken from ``fill_u8`` -- the output of any inpainter, on the page's grid --
    in the gradient domain: the fill's gradients, the level of the page around each hole.  ``page_u8`` and ``fill_u8``: ``[H, W, 3]``
    uint8 of any size; ``mask_u8``: ``[H, W]`` uint8, non-zero = replaced; numpy or torch, none is modified.  One call of the kernel
    (``tsii_seamless_fill``) on the whole page with ``x = page / 255`` and ``out = fill / 255``.  Pixels outside the mask come back byte for
    byte; inside, ``floor(clamp(v, 0, 1) * 255 + 0.5)`` of the blended value, the compose kernels' rounding.  The result is the same
    kind (and on the same device) as ``page_u8``; host arguments are computed on ``device`` (default ``cuda:0``)."""
    sweeps = check_sweeps(sweeps)
    p, m = _page_and_plane(page_u8, mask_u8)
    f = torch.from_numpy(np.ascontiguousarray(fill_u8)) if isinstance(fill_u8, np.ndarray) else fill_u8
    if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8 or tuple(f.shape) != tuple(p.shape):
        raise ValueError(f"fill must be [H, W, 3] uint8 like the page {tuple(p.shape)}, got {tuple(getattr(f, 'shape', ()))} "
                         f"{getattr(f, 'dtype', type(f))}")
    dev = torch.device(device) if device is not None else (p.device if p.is_cuda else torch.device("cuda:0"))
    page, fill, hole = p.to(dev).contiguous(), f.to(dev).contiguous(), m.to(dev) != 0
    x, out = (page.float() / 255.0).unsqueeze(0), (fill.float() / 255.0).unsqueeze(0)
    blended = _seamless_fill(x, out, (~hole).float().unsqueeze(0), sweeps)[0]
    rounded = torch.floor(blended.clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8)
    clean = torch.where(hole.unsqueeze(-1), rounded, page)
    if isinstance(page_u8, np.ndarray):
        return clean.cpu().numpy()
    return clean if clean.device == page_u8.device else clean.to(page_u8.device)


def harmonic_fill(page_u8, mask_u8, sweeps=8, device=None):
    """``clean_u8``: the page with the pixels under the mask replaced by the harmonic fill of their surroundings.  ``page_u8``:
    ``[H, W, 3]`` uint8 of any size; ``mask_u8``: ``[H, W]`` uint8, non-zero = remove (the 255 masks ``TextEraser`` returns work
    directly); numpy or torch, neither is modified.  One call of the kernel on the whole page.  Pixels outside the mask come back byte
    for byte; inside, ``floor(clamp(v, 0, 1) * 255 + 0.5)`` of the filled value, the compose kernels' rounding.  The result is the same
    kind (and on the same device) as ``page_u8``; host arguments are computed on ``device`` (default ``cuda:0``)."""
    sweeps = check_sweeps(sweeps)
    p = torch.from_numpy(np.ascontiguousarray(page_u8)) if isinstance(page_u8, np.ndarray) else page_u8
    m = torch.from_numpy(np.ascontiguousarray(mask_u8)) if isinstance(mask_u8, np.ndarray) else mask_u8
    if p.dim() != 3 or p.shape[2] != 3 or p.dtype != torch.uint8 or p.shape[0] < 1 or p.shape[1] < 1:
        raise ValueError(f"page must be [H, W, 3] uint8, got {tuple(p.shape)} {p.dtype}")
    if m.dtype != torch.uint8 or tuple(m.shape) != tuple(p.shape[:2]):
        raise ValueError(f"mask must be [H, W] uint8 for a page of {tuple(p.shape)}, got {tuple(m.shape)} {m.dtype}")
    dev = torch.device(device) if device is not None else (p.device if p.is_cuda else torch.device("cuda:0"))
    page, hole = p.to(dev).contiguous(), m.to(dev) != 0
    x = (page.float() / 255.0).unsqueeze(0)
    filled = _harmonic_fill(x, (~hole).float().unsqueeze(0), sweeps)[0]
    rounded = torch.floor(filled.clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8)
    clean = torch.where(hole.unsqueeze(-1), rounded, page)
    if isinstance(page_u8, np.ndarray):
        return clean.cpu().numpy()
    return clean if clean.device == page_u8.device else clean.to(page_u8.device)


def patch_fill(page_u8, mask_u8, patch=7, levels=4, iters=4, seed=0, sweeps=8, return_field=False, device=None):
    """``clean_u8``: the page with every pixel under the mask replaced by a COPY of a page pixel outside the mask whose ``patch x patch``
    neighbourhood matches (``tsii_patch_fill`` from ``harmonic_fill(page_u8, mask_u8, sweeps)`` as the first guess; arguments as
    ``PatchFill``).  ``page_u8``: ``[H, W, 3]`` uint8 of any size; ``mask_u8``: ``[H, W]`` uint8, non-zero = remove; numpy or torch,
    neither is modified.  One call of the kernels on the whole page.  Pixels outside the mask come back byte for byte; a pixel under it
    is the harmonic value only where the page has no window free of the mask.  ``return_field=True``: ``(clean_u8, nnf, stats)`` with
    ``nnf`` int32 ``[H, W, 2]``, the ``(y, x)`` every masked pixel was copied from (-1, -1 elsewhere), and ``stats`` int32 ``[3]`` =
    (masked, copied, masked - copied).  The results are the same kind (and on the same device) as ``page_u8``; host arguments are computed
    on ``device`` (default ``cuda:0``)."""
    radius, levels, iters, seed = check_patch_args(patch, levels, iters, seed)
    sweeps = check_sweeps(sweeps)
    p, m = _page_and_plane(page_u8, mask_u8)
    dev = torch.device(device) if device is not None else (p.device if p.is_cuda else torch.device("cuda:0"))
    page, hole = p.to(dev).contiguous(), m.to(dev) != 0
    x = (page.float() / 255.0).unsqueeze(0)
    init = _quantise(_harmonic_fill(x, (~hole).float().unsqueeze(0), sweeps))
    out, nnf, stats = _patch_fill(page.unsqueeze(0), hole.to(torch.uint8).unsqueeze(0), init, radius, levels, iters, seed)
    res = (out[0], nnf[0], stats[0]) if return_field else (out[0],)
    if isinstance(page_u8, np.ndarray):
        res = tuple(t.cpu().numpy() for t in res)
    else:
        res = tuple(t if t.device == page_u8.device else t.to(page_u8.device) for t in res)
    return res if return_field else res[0]
