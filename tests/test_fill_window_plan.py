"""``plan_fill_windows`` (text_segmentation_image_inpainting_amd/pipeline.py): the host step that places the filler's windows on the
text regions for ``TextEraser(pack=True)``.  Pure numpy: no device, no emulator.

``check_contract`` states what the planner promises, with ``S = tile - 2 * halo``:
* the rects cover every input box;
* every rect is non-empty, inside the page, at most ``S`` a side, and inside its window; on each side it keeps ``halo`` pixels to the
  window's edge unless that edge is at or beyond the page's;
* per dimension the origin is in ``[0, side - tile]`` where the page side is at least ``tile``, else ``-((tile - side) // 2)``.
The cases below add hand-built window counts.
"""
import numpy as np
import pytest

import text_segmentation_image_inpainting_amd as T

TILE, HALO = 64, 16
S = TILE - 2 * HALO


def check_contract(boxes, origins, rects, h, w, tile=TILE, halo=HALO):
    s = tile - 2 * halo
    boxes = np.asarray(boxes, np.int64).reshape(-1, 4)
    assert origins.dtype == np.int32 and rects.dtype == np.int32
    assert origins.ndim == 2 and origins.shape[1] == 2 and rects.shape == (len(origins), 4)
    owned = np.zeros((h, w), bool)
    for (oy, ox), (y0, x0, y1, x1) in zip(origins.tolist(), rects.tolist()):
        assert 0 <= y0 < y1 <= h and 0 <= x0 < x1 <= w, "non-empty and inside the page"
        assert y1 - y0 <= s and x1 - x0 <= s
        for o, a, b, side in ((oy, y0, y1, h), (ox, x0, x1, w)):
            assert o <= a and b <= o + tile, "inside its window"
            assert a - o >= halo or o <= 0
            assert o + tile - b >= halo or o + tile >= side
            assert (0 <= o <= side - tile) if side >= tile else (o == -((tile - side) // 2))
        owned[y0:y1, x0:x1] = True
    for y0, x0, y1, x1 in boxes.tolist():
        assert owned[y0:y1, x0:x1].all(), "every box is covered"


def plan(boxes, h, w, tile=TILE, halo=HALO):
    origins, rects = T.plan_fill_windows(np.asarray(boxes, np.int32).reshape(-1, 4), h, w, tile, halo)
    check_contract(boxes, origins, rects, h, w, tile, halo)
    return origins, rects


def test_two_boxes_close_together_share_a_window():
    boxes = [(100, 100, 108, 110), (100, 120, 108, 130)]          # 10 pixels apart
    origins, rects = plan(boxes, 300, 400)
    assert len(origins) == 1 and rects.tolist() == [[100, 100, 108, 130]]
    assert origins.tolist() == [[100 - (TILE - 8) // 2, 100 - (TILE - 30) // 2]], "the window is centred on its rect"


def test_two_boxes_far_apart_get_a_window_each():
    boxes = [(100, 100, 108, 110), (100, 110 + S + 1, 108, 120 + S + 1)]      # S + 1 apart: the union is wider than S
    origins, rects = plan(boxes, 300, 400)
    assert len(origins) == 2 and sorted(rects.tolist()) == sorted(list(b) for b in boxes)


def test_a_box_wider_than_a_core_is_cut():
    box = (50, 40, 80, 140)                                       # 30 rows x 100 columns: wider than S = 32
    origins, rects = plan([box], 300, 400)
    assert len(origins) == 4 and rects.tolist() == [[50, 40 + S * k, 80, min(40 + S * (k + 1), 140)] for k in range(4)]


def test_a_box_in_the_page_corner_clamps_the_origin():
    origins, rects = plan([(0, 0, 6, 9)], 300, 400)
    assert origins.tolist() == [[0, 0]] and rects.tolist() == [[0, 0, 6, 9]]
    origins, rects = plan([(290, 395, 300, 400)], 300, 400)
    assert origins.tolist() == [[300 - TILE, 400 - TILE]] and rects.tolist() == [[290, 395, 300, 400]]


def test_a_page_smaller_than_the_tile_centres_the_window():
    origins, rects = plan([(3, 4, 20, 30)], 40, 50)
    assert origins.tolist() == [[-((TILE - 40) // 2), -((TILE - 50) // 2)]] == [[-12, -7]]
    origins, _ = plan([(0, 0, 40, 50), (5, 5, 6, 6)], 40, 50)    # the whole page: cut into cores, every window the same centred one
    assert len(origins) == 4 and (origins == [-12, -7]).all()


def test_an_empty_table_gives_no_window():
    for boxes in (np.zeros((0, 4), np.int32), []):
        origins, rects = T.plan_fill_windows(boxes, 300, 400, TILE, HALO)
        assert origins.shape == (0, 2) and rects.shape == (0, 4) and origins.dtype == np.int32 and rects.dtype == np.int32


def test_random_boxes_hold_the_contract_and_repeat():
    rng = np.random.default_rng(19)
    h, w = 300, 400
    y0, x0 = rng.integers(0, h - 1, 200), rng.integers(0, w - 1, 200)
    hh, ww = rng.integers(1, 80, 200), rng.integers(1, 120, 200)  # below and above S
    boxes = np.stack([y0, x0, np.minimum(y0 + hh, h), np.minimum(x0 + ww, w)], axis=1).astype(np.int32)
    origins, rects = plan(boxes, h, w)
    again = T.plan_fill_windows(boxes.copy(), h, w, TILE, HALO)
    assert np.array_equal(origins, again[0]) and np.array_equal(rects, again[1])
    assert len(origins) < sum(-(-int(a) // S) * -(-int(b) // S) for a, b in zip(boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1])), \
        "pieces were merged"
    # another geometry: no halo at all, and a tile as large as the page's short side
    plan(boxes, h, w, tile=32, halo=0)
    plan(boxes, h, w, tile=288, halo=40)


def test_bad_boxes_are_refused():
    for box in [(5, 5, 5, 9), (-1, 0, 4, 4), (0, 0, 4, 401)]:
        with pytest.raises(ValueError):
            T.plan_fill_windows([box], 300, 400, TILE, HALO)
