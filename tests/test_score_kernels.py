"""Page scores (csrc/score.hip, include/tsii_hip.h "K18: page scores") through the C ABI on the emulator (CPU suite) and, with -m gpu, on the
chip: the text mask of a (raw, clean) pair (``tsii_pair_text_mask``) and the sums of an eraser's page against the pair
(``tsii_page_scores``).

The semantics, restated.  ``L(p) = (19595 R + 38470 G + 7471 B + 32768) >> 16``; ``t = |L_raw - L_clean| > thr``; ``truth = 255`` where some
``t(y + oy, x + ox)`` on the page holds with ``oy, ox`` in ``-(k // 2) .. k - 1 - k // 2``, else 0.  With ``d = |out - clean|`` per channel,
``a = sum d``, ``s = sum d^2``, ``m = max d``: ``page = (tp, fp, fn, tn of mask != 0 against truth != 0; pixels, sum a, sum s, max m over mask
!= 0; the same over mask == 0)``; row ``r`` of ``rows`` = ``(pixels, sum a, sum s, max m)`` over the pixels labelled ``table[r][0]``.

Everything is an integer: every comparison is EQUALITY with a restatement of another structure than the kernels' (blocks of 64 x 32 pixels,
bit rows in LDS, a per-block table of rows): Pillow's own ``convert("L")`` and ``ImageChops.difference``, a dilation by whole-array
shifts, ``np.bincount`` / ``np.maximum.at`` over ``labels.ravel()``.  Labels and tables come from the fixed-point labelling of
``tests/test_text_regions.py``.  Every output carries a canary tail; the workspace is handed over full of canary bytes, at exactly
``ws_bytes``.
"""
import functools

import numpy as np
import pytest
import torch
from PIL import Image, ImageChops

from tests.backends import BACKENDS, both_backends
from tests.test_flat_kernels import text_of, untouched
from tests.test_pipeline_kernels import Buf, up
from tests.test_text_regions import IDS, expected
from text_segmentation_image_inpainting_amd import _lib, synthetic

PAGES = [(1, 1), (5, 217), (40, 50), (150, 217)]          # the last: more than one 64 x 32 block both ways
KS, THRS = [1, 3, 10, 31], [0, 102, 255]
SLOTS = 32                                                 # SC_SLOTS of csrc/score.hip: the table rows a block of 64 x 32 pixels keeps in LDS


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def shifted(t, oy, ox):
    """out[y, x] = t[y + oy, x + ox] where that is on the page, else 0"""
    h, w = t.shape
    out = np.zeros_like(t)
    ya, yb, xa, xb = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if ya < yb and xa < xb:
        out[ya:yb, xa:xb] = t[ya + oy:yb + oy, xa + ox:xb + ox]
    return out


def pair_ref(raw, clean, thr, k):
    diff = np.asarray(ImageChops.difference(Image.fromarray(raw).convert("L"), Image.fromarray(clean).convert("L")))
    t = diff > thr
    out = np.zeros_like(t)
    for oy in range(-(k // 2), k - 1 - k // 2 + 1):
        for ox in range(-(k // 2), k - 1 - k // 2 + 1):
            out |= shifted(t, oy, ox)
    return out.astype(np.uint8) * 255


def score_ref(out, clean, mask, truth, labels=None, table=None):
    """-> (page int64 [12], rows int64 [n, 4])"""
    d = np.abs(out.astype(np.int64) - clean.astype(np.int64))
    a, s, m = d.sum(axis=-1), (d * d).sum(axis=-1), d.max(axis=-1)
    mk, tr = mask != 0, truth != 0
    page = [(mk & tr).sum(), (mk & ~tr).sum(), (~mk & tr).sum(), (~mk & ~tr).sum()]
    for sel in (mk, ~mk):
        page += [sel.sum(), a[sel].sum(), s[sel].sum(), m[sel].max() if sel.any() else 0]
    if labels is None or table is None or len(table) == 0:
        return np.array(page, np.int64), np.zeros((0, 4), np.int64)
    lab, ids = labels.ravel().astype(np.int64), np.asarray(table)[:, 0].astype(np.int64)
    size = int(max(lab.max(), ids.max())) + 1
    cnt = np.bincount(lab, minlength=size)
    sa = np.bincount(lab, weights=a.ravel(), minlength=size).astype(np.int64)       # float64 sums of integers below 2^53: exact
    ss = np.bincount(lab, weights=s.ravel(), minlength=size).astype(np.int64)
    mx = np.zeros(size, np.int64)
    np.maximum.at(mx, lab, m.ravel())
    rows = np.stack([cnt[ids], sa[ids], ss[ids], mx[ids]], axis=1)
    rows[ids == 0] = 0                                     # label 0 is the background: in no row
    return np.array(page, np.int64), rows.astype(np.int64)


# ---- pages -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_pages(h, w, seed=11):
    """(raw, clean): noise, and the same noise with one pixel in thirty redrawn and one in thirty moved by a few grey levels"""
    rng = np.random.default_rng(seed + h)
    raw = rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8)
    clean = raw.copy()
    redraw, nudge = rng.random((h, w)) < 1 / 30, rng.random((h, w)) < 1 / 30
    clean[redraw] = rng.integers(0, 256, size=(int(redraw.sum()), 3))
    clean[nudge] = np.clip(clean[nudge].astype(np.int16) + rng.integers(-3, 4, size=(int(nudge.sum()), 3)), 0, 255)
    return raw, clean


@functools.lru_cache(maxsize=None)
def score_case(name, h, w, connectivity, seed=5):
    """(out, clean, mask, truth, labels, table, reference): computed once; callers do not modify it.  The mask is the text with one pixel in
    eight flipped, so that all four confusion counts occur and labelled pixels lie on both sides of it"""
    rng = np.random.default_rng(seed + h)
    exp = expected(text_of(name, h, w), connectivity, 0, None)
    out, clean = pair_pages(h, w, seed)
    mask = (((exp["text"] != 0) ^ (rng.random((h, w)) < 1 / 8)) * rng.integers(1, 256, size=(h, w))).astype(np.uint8)
    truth = pair_ref(out, clean, 30, 3)
    return out, clean, mask, truth, exp["labels"], exp["table"], score_ref(out, clean, mask, truth, exp["labels"], exp["table"])


# ---- the kernels -----------------------------------------------------------------------------------------------------------------
def run_pair(dev, raw, clean, thr, k):
    h, w = raw.shape[:2]
    raw_d, clean_d, truth = up(dev, raw), up(dev, clean), Buf(dev, h * w, torch.uint8)
    _lib.call("tsii_pair_text_mask", _lib.ptr(raw_d), _lib.ptr(clean_d), h, w, thr, k, truth.ptr, _lib.stream())
    got = truth.get().reshape(h, w)
    assert np.array_equal(raw_d.cpu().numpy(), raw) and np.array_equal(clean_d.cpu().numpy(), clean), "the pages are read only"
    return got


class Score:
    """the buffers of tsii_page_scores calls on one page"""

    def __init__(self, dev, out, clean, mask, truth, labels=None, table=None, max_rows=None):
        self.h, self.w = mask.shape
        self.inputs = [up(dev, t) for t in (out, clean, mask, truth)]
        self.labels = None if labels is None else up(dev, labels.astype(np.int32))
        self.n = 0 if table is None else len(table)
        self.table = up(dev, np.asarray(table, np.int32).reshape(-1, 6)) if self.n else None
        self.page, self.rows = Buf(dev, 12, torch.int64), Buf(dev, 4 * self.n, torch.int64)
        self.ws_bytes = _lib.lib().tsii_page_scores_ws_bytes(self.h, self.w, self.n if max_rows is None else max_rows)
        assert self.ws_bytes == 4 * 12 * (-(-self.h // 32)) * (-(-self.w // 64))
        self.ws = Buf(dev, self.ws_bytes // 4, torch.int32)

    def run(self, **bad):
        a = dict(zip(("out", "clean", "mask", "truth"), map(_lib.ptr, self.inputs)), labels=_lib.ptr(self.labels), table=_lib.ptr(self.table),
                 n=self.n, h=self.h, w=self.w, page=self.page.ptr, rows=self.rows.ptr, ws=self.ws.ptr, ws_bytes=self.ws_bytes)
        a.update(bad)
        _lib.call("tsii_page_scores", a["out"], a["clean"], a["mask"], a["truth"], a["labels"], a["table"], a["n"], a["h"], a["w"], a["page"],
                  a["rows"], a["ws"], a["ws_bytes"], _lib.stream())

    def get(self):
        self.ws.get()
        return self.page.get(), self.rows.get().reshape(-1, 4)


def run_score(backend, out, clean, mask, truth, labels=None, table=None, ref=None, twice=False):
    ref = score_ref(out, clean, mask, truth, labels, table) if ref is None else ref
    with BACKENDS[backend]() as dev:
        sc = Score(dev, out, clean, mask, truth, labels, table)
        sc.run()
        got = sc.get()
        if twice:                                          # the same buffers, what the first call left in them included
            sc.run()
            again = sc.get()
        after = [t.cpu().numpy() for t in sc.inputs]
    assert np.array_equal(got[0], ref[0]), (got[0], ref[0])
    assert np.array_equal(got[1], ref[1]), int((got[1] != ref[1]).any(axis=1).sum())
    assert not twice or (np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1]))
    assert all(np.array_equal(x, y) for x, y in zip(after, (out, clean, mask, truth))), "the inputs are read only"
    return ref


# ---- the pair's mask ---------------------------------------------------------------------------------------------------------------
def test_luma_is_pillows():
    """the integer form of the header against Pillow's convert("L") on every value of each channel and on noise"""
    ramp = np.zeros((3, 256, 3), np.uint8)
    for c in range(3):
        ramp[c, :, c] = np.arange(256)
    for img in (ramp, 255 - ramp, pair_pages(150, 217)[0]):
        v = img.astype(np.int64)
        assert np.array_equal((19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 32768) >> 16, np.asarray(Image.fromarray(img).convert("L")))


@both_backends
@pytest.mark.parametrize("thr", THRS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("hw", PAGES, **IDS)
def test_pair_text_mask(backend, hw, k, thr):
    raw, clean = pair_pages(*hw)
    ref = pair_ref(raw, clean, thr, k)
    with BACKENDS[backend]() as dev:
        got = run_pair(dev, raw, clean, thr, k)
    assert np.array_equal(got, ref), int((got != ref).sum())
    if k == 10:
        t = np.asarray(ImageChops.difference(Image.fromarray(raw).convert("L"), Image.fromarray(clean).convert("L"))) > thr
        assert np.array_equal(got, synthetic.dilate_10x10(t.astype(np.uint8) * 255))
    if thr == 255:
        assert not got.any()
    elif hw == (150, 217) and k <= 3:                      # one pixel in fifteen differs: a 31 x 31 square around each covers the page
        assert 0 < (got != 0).mean() < 1


@both_backends
@pytest.mark.parametrize("k", [2, 10, 31])
@pytest.mark.parametrize("hw", PAGES[2:], **IDS)
def test_pair_anchor(backend, hw, k):
    """one differing pixel in each corner and in the middle: the square reaches k // 2 up and left and k - 1 - k // 2 down and right, and the
    page edge cuts it"""
    h, w = hw
    raw = np.full((h, w, 3), 200, np.uint8)
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)):
        clean = raw.copy()
        clean[y, x] = (90, 90, 90)
        with BACKENDS[backend]() as dev:
            got = run_pair(dev, raw, clean, 102, k)
        ref = np.zeros((h, w), np.uint8)
        ref[max(0, y - (k - 1 - k // 2)):y + k // 2 + 1, max(0, x - (k - 1 - k // 2)):x + k // 2 + 1] = 255
        assert np.array_equal(got, ref), (y, x, int((got != ref).sum()))
        assert np.array_equal(got, pair_ref(raw, clean, 102, k))


@both_backends
def test_pair_threshold_is_strict(backend):
    """|L_raw - L_clean| of exactly thr is no text, thr + 1 is"""
    raw = np.full((3, 4, 3), 150, np.uint8)
    clean = raw.copy()
    clean[1, 1], clean[1, 2] = 48, 47                     # grey: L is the grey level; differences of 102 and 103
    assert np.asarray(Image.fromarray(clean).convert("L"))[1, 1:3].tolist() == [48, 47]
    with BACKENDS[backend]() as dev:
        got = run_pair(dev, raw, clean, 102, 1)
    assert np.argwhere(got).tolist() == [[1, 2]] and got[1, 2] == 255


# ---- the scores --------------------------------------------------------------------------------------------------------------------
@both_backends
@pytest.mark.parametrize("name,connectivity", [("blocks", 8), ("noise0.3", 4), ("noise0.45", 8), ("full", 8), ("empty", 8)])
@pytest.mark.parametrize("hw", PAGES, **IDS)
def test_scores(backend, hw, name, connectivity):
    """random pages; the noise patterns put hundreds of regions into one block, far more than its table holds"""
    out, clean, mask, truth, labels, table, ref = score_case(name, *hw, connectivity)
    run_score(backend, out, clean, mask, truth, labels, table, ref)
    if hw == (150, 217):
        assert all(v > 0 for v in ref[0]), "every count and every sum of the page is exercised"
        if name == "noise0.3":
            first_block = np.unique(labels[:32, :64])
            assert len(first_block) - 1 > 8 * SLOTS and len(table) > 2000


@both_backends
def test_more_rows_in_a_block_than_slots(backend):
    """ONE block of 64 x 32 pixels with 512 single-pixel regions, each with an error of its own: the block's LDS table holds SLOTS = 32 rows,
    the other 480 go to memory run by run; then the same with exactly SLOTS regions and with SLOTS + 1"""
    h, w = 32, 64
    rng = np.random.default_rng(3)
    out, clean = rng.integers(0, 256, size=(2, h, w, 3)).astype(np.uint8)
    for count in (512, SLOTS, SLOTS + 1):
        text = np.zeros((h, w), np.uint8)
        ys, xs = np.mgrid[0:h:2, 0:w:2]
        text[ys.ravel()[:count], xs.ravel()[:count]] = 1
        exp = expected(text, 8, 0, None)
        assert len(exp["table"]) == count
        _, rows = run_score(backend, out, clean, text * 255, text * 255, exp["labels"], exp["table"])
        assert (rows[:, 0] == 1).all() and len(np.unique(rows[:, 1])) > 20


@both_backends
@pytest.mark.parametrize("hw", PAGES[1:], **IDS)
def test_without_rows(backend, hw):
    """labels NULL; n_rows = 0 with labels; both: only `page` is written"""
    out, clean, mask, truth, labels, table, ref = score_case("blocks", *hw, 8)
    page_only = (ref[0], np.zeros((0, 4), np.int64))
    run_score(backend, out, clean, mask, truth, None, None, page_only)
    run_score(backend, out, clean, mask, truth, labels, None, page_only)
    with BACKENDS[backend]() as dev:
        sc = Score(dev, out, clean, mask, truth, None, table)         # a table and rows, but no labels: the rows keep their canary
        sc.run()
        page, rows = sc.get()
    assert np.array_equal(page, ref[0]) and untouched(rows)


@both_backends
def test_rows_and_tables_that_do_not_match(backend):
    """a table row whose label does not occur is all zero; labelled pixels whose label is not in the table count in no row"""
    out, clean, mask, truth, labels, table, ref = score_case("blocks", 150, 217, 8)
    absent = np.array([[2, 9, 0, 0, 1, 1], [labels.max() - 1, 9, 0, 0, 1, 1], [150 * 217 + 1, 9, 0, 0, 1, 1]], np.int32)
    assert not np.isin(absent[:, 0], labels).any()
    grown = np.concatenate([table, absent])
    grown = grown[np.argsort(grown[:, 0], kind="stable")]
    _, rows = run_score(backend, out, clean, mask, truth, labels, grown)
    assert (rows[np.isin(grown[:, 0], absent[:, 0])] == 0).all() and (rows[~np.isin(grown[:, 0], absent[:, 0])][:, 0] > 0).all()
    thinned = table[::3]
    _, rows = run_score(backend, out, clean, mask, truth, labels, thinned)
    assert np.array_equal(rows, ref[1][::3]) and rows[:, 0].sum() < (labels != 0).sum()


@both_backends
@pytest.mark.parametrize("hw", PAGES, **IDS)
def test_extremes(backend, hw):
    """out all 0 against clean all 255: the largest sums a page of this size has; the mask all 0 and all 255"""
    h, w = hw
    exp = expected(text_of("blocks", h, w), 8, 0, None)
    out, clean = np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)
    truth = (exp["text"] != 0).astype(np.uint8)
    for mask in (np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)):
        page, rows = run_score(backend, out, clean, mask, truth, exp["labels"], exp["table"])
        side = 4 if mask.any() else 8
        assert page[side:side + 4].tolist() == [h * w, h * w * 765, h * w * 3 * 255 * 255, 255] and not page[12 - side:16 - side].any()
        assert np.array_equal(rows, np.outer(exp["table"][:, 1], [1, 765, 3 * 255 * 255, 0]) + [0, 0, 0, 255])
    raw, clean = pair_pages(h, w)
    for mask in (np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)):
        run_score(backend, raw, clean, mask, truth, exp["labels"], exp["table"])


@both_backends
@pytest.mark.parametrize("hw", PAGES[2:], **IDS)
def test_scored_twice(backend, hw):
    """the same buffers scored twice give the same bytes: the call clears what it accumulates into"""
    out, clean, mask, truth, labels, table, ref = score_case("noise0.45", *hw, 8)
    run_score(backend, out, clean, mask, truth, labels, table, ref, twice=True)


@both_backends
def test_refusals(backend):
    out, clean, mask, truth, labels, table, _ = score_case("blocks", 40, 50, 8)
    lib = _lib.lib
    with BACKENDS[backend]() as dev:
        assert lib().tsii_page_scores_ws_bytes(0, 5, 1) == 0 and lib().tsii_page_scores_ws_bytes(5, 0, 1) == 0
        assert lib().tsii_page_scores_ws_bytes(5, 5, -1) == 0 and lib().tsii_page_scores_ws_bytes(46341, 46341, 1) == 0
        assert lib().tsii_page_scores_ws_bytes(2 ** 31 - 2, 1, 0) == 48 * 2 ** 26 and lib().tsii_page_scores_ws_bytes(1, 2 ** 31 - 1, 0) == 0
        assert lib().tsii_page_scores_ws_bytes(33, 65, 7) == 48 * 4
        sc = Score(dev, out, clean, mask, truth, labels, table)
        for bad in [dict(h=0), dict(w=0), dict(h=46341, w=46341), dict(n=-1), dict(out=None), dict(clean=None), dict(mask=None), dict(truth=None),
                    dict(page=None), dict(ws=None), dict(table=None), dict(rows=None), dict(ws_bytes=sc.ws_bytes - 1), dict(ws_bytes=0)]:
            with pytest.raises(RuntimeError, match=r"tsii_page_scores failed \(-?[1-9]\d*\): "):
                sc.run(**bad)
        with pytest.raises(RuntimeError, match="workspace"):
            sc.run(ws_bytes=sc.ws_bytes - 4)
        raw_d, clean_d, truth_b = up(dev, out), up(dev, clean), Buf(dev, 40 * 50, torch.uint8)
        for bad in [dict(h=0), dict(w=0), dict(h=46341, w=46341), dict(thr=-1), dict(thr=256), dict(k=0), dict(k=32), dict(raw=None), dict(clean=None),
                    dict(truth=None), dict(truth=_lib.ptr(raw_d))]:
            a = dict(raw=_lib.ptr(raw_d), clean=_lib.ptr(clean_d), h=40, w=50, thr=102, k=10, truth=truth_b.ptr)
            a.update(bad)
            with pytest.raises(RuntimeError, match=r"tsii_pair_text_mask failed \(-?[1-9]\d*\): "):
                _lib.call("tsii_pair_text_mask", a["raw"], a["clean"], a["h"], a["w"], a["thr"], a["k"], a["truth"], _lib.stream())
        outputs = [sc.page.get(), sc.rows.get(), sc.ws.get(), truth_b.get()]
        pages_after = [raw_d.cpu().numpy(), clean_d.cpu().numpy()]
    assert all(untouched(a) for a in outputs), "a refused call must not write"
    assert np.array_equal(pages_after[0], out) and np.array_equal(pages_after[1], clean)


def test_foreign_table_stays_inside_the_buffers():
    """EMULATOR ONLY: labels the table does not know, labels of any sign and size, a table that does not ascend: wrong numbers, and every
    canary intact"""
    out, clean, mask, truth, labels, _, _ = score_case("noise0.45", 40, 50, 8)
    big = 2 ** 31 - 1
    rng = np.random.default_rng(9)
    wild = labels.copy()
    sel = rng.random(labels.shape) < 0.3
    wild[sel] = rng.integers(-big, big, size=int(sel.sum()))
    wild[0, :8] = [big, -big - 1, -1, 1, 0, 2000, 2001, -7]
    tables = [[[k * 7 - 20, 1, -big, -big, big, big] for k in range(16)], [[5, 1, 0, 0, 1, 1]] * 16, [[big - k, 1, 0, 0, 1, 1] for k in range(16)],
              [[-big - 1 + k, 1, 0, 0, 1, 1] for k in range(40)]]
    with BACKENDS["emu"]() as dev:
        for table in tables:
            for lab in (labels, wild):
                sc = Score(dev, out, clean, mask, truth, lab, np.array(table, np.int64).astype(np.int32))
                sc.run()
                page, rows = sc.get()
                assert np.array_equal(page, score_ref(out, clean, mask, truth)[0]) and rows[:, 0].sum() <= 40 * 50 and (rows >= 0).all()
