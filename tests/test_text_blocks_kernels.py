"""Text blocks (csrc/blocks.hip, include/tsii_hip.h "K15: text blocks"): single-linkage grouping of the components of a label plane at
Chebyshev distance ``gap``, through the C ABI on the emulator (CPU suite) and, with -m gpu, on the chip.

Everything is integer: every comparison is EQUALITY with a restatement that does not share the kernels' mechanism (no dilated plane, no
labelling of one).  The components come from ``tests/test_text_regions.py``'s fixed-point labelling; the blocks from min-label
propagation over the labelled pixels: every pixel takes the smallest label within Chebyshev distance ``gap`` of it (a separable
minimum filter of radius ``gap``, the background at +inf) and the value of the pixel its value names, until nothing changes.  On planes
of at most ~2000 text pixels a second restatement -- the pairwise Chebyshev matrix and union-find over the components -- has to agree
with the first.  Every buffer carries a canary tail; the workspace is handed over full of canary bytes.
"""
import functools

import numpy as np
import pytest
import torch

from tests.backends import BACKENDS, both_backends
from tests.test_pipeline_kernels import CANARY, Buf
from tests.test_text_regions import expected as regions_expected
from tests.test_text_regions import pattern
from text_segmentation_image_inpainting_amd import _lib
from text_segmentation_image_inpainting_amd.pipeline import tile_grid

TILE, HALO = 64, 8
PAGES = [(1, 1), (1, 37), (37, 1), (40, 50), (150, 217), (300, 420)]
GAPS = [1, 2, 3, 8, 33, 64]
CANARY32 = int(np.frombuffer(bytes([CANARY] * 4), np.int32)[0])
IDS = dict(ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def min_filter(a, radius, axis, big):
    """minimum over the window [-radius, +radius] along ``axis``; beyond the array: ``big``"""
    n = a.shape[axis]
    pad = [(0, 0), (0, 0)]
    pad[axis] = (radius, radius)
    p = np.pad(a, pad, constant_values=big)
    cov = 1                                             # p[i] = min over the cov entries from i on
    while cov < 2 * radius + 1:
        s = min(cov, 2 * radius + 1 - cov)
        q = np.full_like(p, big)
        sl_to, sl_from = [slice(None)] * 2, [slice(None)] * 2
        sl_to[axis], sl_from[axis] = slice(0, p.shape[axis] - s), slice(s, None)
        q[tuple(sl_to)] = p[tuple(sl_from)]
        p = np.minimum(p, q)
        cov += s
    sl = [slice(None)] * 2
    sl[axis] = slice(0, n)
    return p[tuple(sl)]


def block_plane(labels, gap):
    """int64 [h,w]: the smallest label within reach of each labelled pixel's block, 0 off the labelled pixels"""
    h, w = labels.shape
    fg = labels != 0
    big = np.int64(h * w + 1)
    lab = np.where(fg, labels.astype(np.int64), big)
    while True:
        new = min_filter(min_filter(lab, gap, 0, big), gap, 1, big)
        new = np.where(fg, new, big)
        named = np.append(new.reshape(-1), big)[np.minimum(new, big) - 1].reshape(h, w)      # a label names a pixel of its own block
        new = np.where(fg, np.minimum(new, named), big)
        if np.array_equal(new, lab):
            return np.where(fg, lab, 0)
        lab = new


def block_plane_brute(labels, gap):
    """the same from the pairwise Chebyshev matrix of the labelled pixels and union-find over the components"""
    ys, xs = np.nonzero(labels)
    assert len(ys) <= 2500
    comp = labels[ys, xs].astype(np.int64)
    near = np.maximum(np.abs(ys[:, None] - ys[None, :]), np.abs(xs[:, None] - xs[None, :])) <= gap
    i, j = np.nonzero(near)
    base = np.int64(labels.size + 1)
    codes = np.unique(comp[i] * base + comp[j])
    pairs = np.stack([codes // base, codes % base], axis=1)
    parent = {int(c): int(c) for c in np.unique(comp)}

    def find(c):
        while parent[c] != c:
            parent[c] = parent[parent[c]]
            c = parent[c]
        return c
    for a, b in pairs.tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)            # the smaller label is the root: the block's label
    out = np.zeros(labels.shape, np.int64)
    out[ys, xs] = [find(int(c)) for c in comp]
    return out


def expected(text, labels, gap, min_area, g):
    """-> dict(labels, text, n, table, members (every kept row), core); ``text`` only gives the shape: the labels decide"""
    h, w = labels.shape
    full = block_plane(labels, gap)
    if int((labels != 0).sum()) <= 2000:
        assert np.array_equal(full, block_plane_brute(labels, gap)), "the two restatements disagree"
    ids, area = np.unique(full[full > 0], return_counts=True)
    pairs = np.unique(np.stack([full[full > 0], labels[full > 0].astype(np.int64)], axis=1), axis=0)
    nmemb = np.array([(pairs[:, 0] == b).sum() for b in ids], np.int64)
    keep = area >= min_area
    kept = ids[keep]
    out_labels = np.where(np.isin(full, kept), full, 0)
    ys, xs = np.nonzero(out_labels)
    _, inv = np.unique(out_labels[ys, xs], return_inverse=True)
    y0, x0, y1, x1 = (np.full(len(kept), v, np.int64) for v in (h, w, 0, 0))
    np.minimum.at(y0, inv, ys), np.minimum.at(x0, inv, xs), np.maximum.at(y1, inv, ys + 1), np.maximum.at(x1, inv, xs + 1)
    rows = np.stack([kept, area[keep], y0, x0, y1, x1], axis=1) if len(kept) else []
    out = (out_labels != 0).astype(np.uint8)
    core = None if g is None else np.array([out[a:b, c:d].sum() for (a, b, c, d) in map(g.core, range(g.count))], np.int32)
    return dict(labels=out_labels.astype(np.int32), text=out, n=(len(ids), len(kept)), table=np.array(rows, np.int32).reshape(-1, 6),
                members=nmemb[keep].astype(np.int32), core=core)


def k10_labels(text, connectivity=8):
    """what tsii_text_regions leaves for ``text`` with min_area = 0 (its own tests hold the kernels to this)"""
    return regions_expected(text, connectivity, 0, None)["labels"]


# ---- the kernels -----------------------------------------------------------------------------------------------------------------
class Planes:
    """the buffers of one call, every one with a canary tail; the workspace is full of canary bytes"""

    def __init__(self, dev, text, labels, gap, max_regions, g):
        h, w = labels.shape
        self.h, self.w, self.g, self.gap, self.max_regions = h, w, g, gap, max_regions
        self.text, self.labels = Buf(dev, h * w, torch.uint8), Buf(dev, h * w, torch.int32)
        self.text.raw[:h * w] = torch.from_numpy(np.ascontiguousarray(text).reshape(-1)).to(dev)
        self.labels.raw[:4 * h * w] = torch.from_numpy(np.ascontiguousarray(labels, np.int32).reshape(-1)).view(torch.uint8).to(dev)
        self.blocks, self.n = Buf(dev, h * w, torch.int32), Buf(dev, 2, torch.int32)
        self.table = Buf(dev, 6 * max_regions, torch.int32) if max_regions else None
        self.members = Buf(dev, max_regions, torch.int32) if max_regions else None
        self.core = Buf(dev, g.count, torch.int32) if g is not None else None
        nbytes = _lib.lib().tsii_text_blocks_ws_bytes(h, w, max_regions, gap)
        assert nbytes > 0 and nbytes % 8 == 0
        self.ws = Buf(dev, nbytes // 4, torch.int32)

    def run(self, min_area=0, tile=TILE, halo=HALO, gap=None, blocks_ptr=None, **null):
        assert all(v is True for v in null.values()) and set(null) <= {"text", "labels", "blocks", "table", "members", "n", "ws"}, null
        p = lambda name, buf: None if (buf is None or null.get(name)) else buf.ptr
        _lib.call("tsii_text_blocks", p("text", self.text), p("labels", self.labels), self.h, self.w, self.gap if gap is None else gap, min_area,
                  self.max_regions, tile, halo, p("core", self.core), blocks_ptr if blocks_ptr is not None else p("blocks", self.blocks),
                  p("table", self.table), p("members", self.members), p("n", self.n), p("ws", self.ws), _lib.stream())

    def get(self):
        self.ws.get()                                    # the canary behind the workspace
        return dict(labels=self.blocks.get().reshape(self.h, self.w), text=self.text.get().reshape(self.h, self.w), n=tuple(self.n.get()),
                    table=self.table.get().reshape(-1, 6) if self.table else np.zeros((0, 6), np.int32),
                    members=self.members.get() if self.members else np.zeros(0, np.int32),
                    core=self.core.get() if self.core else None, input=self.labels.get().reshape(self.h, self.w))


def check(got, exp, max_regions, labels):
    assert got["n"] == exp["n"], (got["n"], exp["n"])
    assert np.array_equal(got["labels"], exp["labels"]), int((got["labels"] != exp["labels"]).sum())
    assert np.array_equal(got["text"], exp["text"])
    assert np.array_equal(got["input"], labels), "the label plane is read only"
    n = min(exp["n"][1], max_regions)
    assert np.array_equal(got["table"][:n], exp["table"][:n])
    assert np.array_equal(got["members"][:n], exp["members"][:n]), (got["members"][:n], exp["members"][:n])
    assert bool((got["table"][n:] == CANARY32).all()) and bool((got["members"][n:] == CANARY32).all()), "rows behind the kept blocks must not be touched"
    if exp["core"] is not None:
        assert np.array_equal(got["core"], exp["core"]), (got["core"], exp["core"])


def run_plane(dev, text, gap, connectivity=8, min_area=0, max_regions=None, tiled=True, labels=None):
    """one call on ``text`` (labels: K10's, unless given) -> the expectation it was held to"""
    text = np.ascontiguousarray(text, np.uint8)
    labels = k10_labels(text, connectivity) if labels is None else labels
    g = tile_grid(*text.shape, TILE, HALO) if tiled else None
    exp = expected(text, labels, gap, min_area, g)
    max_regions = exp["n"][1] + 3 if max_regions is None else max_regions
    planes = Planes(dev, text, labels, gap, max_regions, g)
    planes.run(min_area)
    check(planes.get(), exp, max_regions, labels)
    return exp


@functools.lru_cache(maxsize=None)
def pattern_case(name, h, w, gap):
    """(text, labels, expectation): computed once, shared by the backends; callers do not modify it"""
    text = pattern(name, h, w)
    labels = k10_labels(text)
    return text, labels, expected(text, labels, gap, 0, tile_grid(h, w, TILE, HALO))


@both_backends
@pytest.mark.parametrize("gap", GAPS)
@pytest.mark.parametrize("name", ["noise0.002", "noise0.02", "noise0.3", "full", "empty"])
@pytest.mark.parametrize("hw", PAGES, **IDS)
def test_patterns(backend, hw, name, gap):
    text, labels, exp = pattern_case(name, *hw, gap)
    h, w = hw
    with BACKENDS[backend]() as dev:
        planes = Planes(dev, text, labels, gap, exp["n"][1] + 3, tile_grid(h, w, TILE, HALO))
        planes.run()
        got = planes.get()
    check(got, exp, exp["n"][1] + 3, labels)
    if name == "full":
        assert exp["n"] == (1, 1) and tuple(exp["table"][0]) == (1, h * w, 0, 0, h, w) and exp["members"][0] == 1
    if name == "empty":
        assert exp["n"] == (0, 0) and not exp["core"].any()


def test_noise_planes_have_many_blocks():
    """the sparse planes are not one block or all singletons: the comparison above means something"""
    for gap in (2, 8):
        exp = pattern_case("noise0.002", 300, 420, gap)[2]
        assert 20 < exp["n"][0] and int(exp["members"].max()) > 1, exp["n"]


DIRECTIONS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


@both_backends
@pytest.mark.parametrize("gap", GAPS)
def test_distance_in_eight_directions(backend, gap):
    """two pixels exactly ``gap`` apart are one block, ``gap + 1`` apart two; diagonals and mixed offsets included"""
    h = w = 2 * (gap + 1) + 3                            # room for gap + 1 either way of the centre
    cy = cx = gap + 2
    with BACKENDS[backend]() as dev:
        for dy, dx in DIRECTIONS:
            for dist, blocks in ((gap, 1), (gap + 1, 2)):
                text = np.zeros((h, w), np.uint8)
                text[cy, cx] = text[cy + dy * dist, cx + dx * dist] = 1
                exp = run_plane(dev, text, gap)
                assert exp["n"] == (blocks, blocks) and list(exp["members"]) == ([2 if dist > 1 else 1] if blocks == 1 else [1, 1]), (dy, dx, dist)   # 1 apart: one component
        for off, blocks in (((gap, 1), 1), ((1, gap), 1), ((gap + 1, 0), 2), ((gap // 2, gap + 1), 2)):
            text = np.zeros((h, w), np.uint8)
            text[cy, cx] = text[cy - off[0], cx + off[1]] = 1
            assert run_plane(dev, text, gap)["n"][0] == blocks, off


@both_backends
@pytest.mark.parametrize("gap", GAPS)
def test_chain(backend, gap):
    """A - B - C: A and C are 2 * gap apart and still one block, through B; a fourth component one pixel too far is its own"""
    text = np.zeros((150, 217), np.uint8)
    text[10, 5] = text[10 + gap, 5 + gap] = text[10 + 2 * gap, 5 + gap] = 1
    text[10 + 2 * gap, 5 + 2 * gap + 1] = 1
    with BACKENDS[backend]() as dev:
        exp = run_plane(dev, text, gap)
    assert exp["n"] == (2, 2) and list(exp["members"]) == [3 if gap > 1 else 1, 1] and exp["table"][0][1] == 3      # gap 1: K10 joins A, B, C itself


@both_backends
@pytest.mark.parametrize("gap", GAPS)
def test_across_word_and_tile_boundaries(backend, gap):
    """pairs exactly ``gap`` (one block) and ``gap + 1`` (two) apart on either side of columns 31/32, 63/64, 255/256 and rows 31/32, 63/64:
    the word, rectangle and tile edges of the packing, dilating and labelling kernels"""
    with BACKENDS[backend]() as dev:
        for axis, edge in ((1, 32), (1, 64), (1, 256), (0, 32), (0, 64)):
            for dist, blocks in ((gap, 1), (gap + 1, 2)):
                first = max(0, edge - (dist + 1) // 2)      # first < edge <= first + dist
                text = np.zeros((9, 330) if axis else (110, 9), np.uint8)
                a, b = [4, 4], [4, 4]
                a[axis], b[axis] = first, first + dist
                text[a[0], a[1]] = text[b[0], b[1]] = 1
                exp = run_plane(dev, text, gap)
                assert exp["n"][0] == blocks and set(exp["members"]) == ({2 if dist > 1 else 1} if blocks == 1 else {1}), (axis, edge, dist)


@both_backends
@pytest.mark.parametrize("gap", GAPS)
@pytest.mark.parametrize("hw", [(1, 37), (37, 1), (40, 50), (150, 217)], **IDS)
def test_border_and_corners(backend, hw, gap):
    h, w = hw
    text = np.zeros(hw, np.uint8)
    for y in (0, h // 2, h - 1):
        for x in (0, w // 2, w - 1):
            text[y, x] = 1
    with BACKENDS[backend]() as dev:
        exp = run_plane(dev, text, gap)
    assert exp["n"][0] >= 1 and int(exp["members"].sum()) == int(text.sum())


@both_backends
def test_four_connected_labels_with_diagonal_neighbours(backend):
    """connectivity = 4 makes diagonal neighbours different components; at gap = 1 they are one block"""
    text = np.zeros((40, 50), np.uint8)
    for k in range(6):
        text[10 + k, 20 + k] = 1
    text[30, 5] = text[31, 6] = 1
    with BACKENDS[backend]() as dev:
        exp = run_plane(dev, text, 1, connectivity=4)
    assert exp["n"] == (2, 2) and list(exp["members"]) == [6, 2] and list(exp["table"][:, 1]) == [6, 2]


def min_area_plane():
    text = np.zeros((150, 217), np.uint8)
    text[60, 60:62] = text[60, 65:67] = text[64, 62:64] = 1          # three 2-pixel components, each within 4 of another
    text[100:102, 150:152] = 1                                       # a lone 4-pixel component
    return text


@both_backends
@pytest.mark.parametrize("tiled", [True, False], ids=["core_count", "no_core_count"])
def test_min_area_judges_blocks(backend, tiled):
    text = min_area_plane()
    with BACKENDS[backend]() as dev:
        exp = run_plane(dev, text, 4, min_area=5, tiled=tiled)
        everything = run_plane(dev, text, 4, min_area=1, tiled=tiled)
    assert exp["n"] == (2, 1) and list(exp["members"]) == [3] and tuple(exp["table"][0][1:]) == (6, 60, 60, 65, 67)
    assert exp["text"].sum() == 6 and not exp["text"][100:102].any() and not exp["labels"][100:102].any()
    assert everything["n"] == (2, 2) and everything["text"].sum() == 10
    if tiled:
        assert exp["core"].sum() == 6 and everything["core"].sum() == 10


@both_backends
def test_unlabelled_text_is_background(backend):
    """text != 0 over labels == 0 (a region K10's own filter dropped): no component, and the text byte is rewritten to 0"""
    text = np.zeros((40, 50), np.uint8)
    text[5, 5:9] = 7
    text[5, 12] = 255                                                # would bridge to (5, 15) at gap 3 if it counted
    text[5, 15:18] = 1
    labels = k10_labels(text)
    labels[labels == labels[5, 12]] = 0
    with BACKENDS[backend]() as dev:
        exp = run_plane(dev, text, 3, labels=labels)
    assert exp["n"] == (2, 2) and exp["text"][5, 12] == 0 and exp["text"].sum() == 7


@both_backends
def test_truncated_table(backend):
    """more kept blocks than rows: the first max_regions rows in label order, the rows behind them untouched, the true count"""
    text = np.zeros((150, 217), np.uint8)
    text[::10, ::10] = 1
    with BACKENDS[backend]() as dev:
        exp = run_plane(dev, text, 3, max_regions=100)
        run_plane(dev, text, 3, max_regions=0)                       # no table at all (table == NULL, members == NULL)
    assert exp["n"] == (15 * 22, 15 * 22) and np.array_equal(exp["table"][:3, 0], [1, 11, 21])


@both_backends
def test_same_workspace_twice(backend):
    """the second call reuses the first call's workspace as it was left: identical outputs"""
    text, labels, _ = pattern_case("noise0.02", 150, 217, 8)
    g = tile_grid(150, 217, TILE, HALO)
    exp = expected(text, labels, 8, 5, g)
    with BACKENDS[backend]() as dev:
        a = Planes(dev, text, labels, 8, 4096, g)
        a.run(5)
        first = a.get()
        b = Planes(dev, text, labels, 8, 4096, g)
        b.ws = a.ws
        b.run(5)
        second = b.get()
    check(first, exp, 4096, labels)
    check(second, exp, 4096, labels)


@both_backends
def test_refusals(backend):
    text = pattern("noise0.02", 40, 50)
    labels = k10_labels(text)
    ws_bytes = _lib.lib().tsii_text_blocks_ws_bytes
    with BACKENDS[backend]() as dev:
        assert ws_bytes(46341, 46341, 1, 3) == 0 and ws_bytes(0, 5, 1, 3) == 0 and ws_bytes(5, 5, -1, 3) == 0
        assert ws_bytes(5, 5, 1, 0) == 0 and ws_bytes(5, 5, 1, 65) == 0 and ws_bytes(5, 5, 1, 64) > 0
        p = Planes(dev, text, labels, 3, 16, tile_grid(40, 50, TILE, HALO))
        for gap in (0, -1, 65):
            with pytest.raises(RuntimeError, match=r"tsii_text_blocks failed \(-?[1-9]\d*\): .*gap"):
                p.run(gap=gap)
        for name in ("text", "labels", "blocks", "n", "ws"):
            with pytest.raises(RuntimeError, match="null"):
                p.run(**{name: True})
        for name in ("table", "members"):
            with pytest.raises(RuntimeError, match="max_regions"):
                p.run(**{name: True})
        with pytest.raises(RuntimeError, match="label plane itself"):
            p.run(blocks_ptr=p.labels.ptr)
        with pytest.raises(RuntimeError, match="geometry"):
            p.run(tile=48, halo=4)
        with pytest.raises(RuntimeError, match="geometry"):
            p.run(tile=64, halo=32)
        p.max_regions = -1
        with pytest.raises(RuntimeError, match="max_regions"):
            p.run()
        got = p.get()
        ws = p.ws.get()
    assert np.array_equal(got["text"], text) and np.array_equal(got["input"], labels), "a refused call must not touch its planes"
    for name in ("labels", "n", "table", "members", "core"):
        assert bool((np.asarray(got[name]) == CANARY32).all()), name
    assert bool((ws == CANARY32).all())
