"""``region_geometry`` and the helpers of ``RegionGeometry`` (``regions.py``; the kernels: tests/test_region_geometry.py, whose restatement
and patterns this file uses).  The integers are compared for equality; the helpers are floating point on top of them and are held to what
they promise: every pixel centre lies inside ``box_points`` within 1e-9, every pixel square inside ``box_points(pad=True)``, the sides
multiply to the rectangle's area, the angle is the longer side's.  Every kernel case runs on the emulator (CPU suite) and, with -m gpu, on
the chip.
"""
import numpy as np
import pytest
import torch

import text_segmentation_image_inpainting_amd as T
from tests.backends import BACKENDS, both_backends
from tests.test_region_geometry import case, expected_geometry, geometry_pattern

PATTERNS = [("pixel", 40, 50), ("row", 5, 217), ("column", 150, 3), ("diagonal", 40, 50), ("stair3", 40, 51), ("box", 40, 50),
            ("disc40", 150, 217), ("tilted", 150, 217), ("L", 40, 50), ("C", 40, 50), ("two_L", 40, 50), ("noise0.35", 40, 50)]


def check_against(r, exp, exp_geo, max_vertices, rows=None):
    rows = len(exp_geo) if rows is None else rows
    assert r.n_vertices.dtype == np.int32 and r.vertices.dtype == np.int32 and r.rect.dtype == np.int64
    assert r.n_vertices.shape == (rows,) and r.vertices.shape == (rows, max_vertices, 2) and r.rect.shape == (rows, 8)
    for k, (verts, box) in enumerate(exp_geo[:rows]):
        n = min(len(verts), max_vertices)
        assert int(r.n_vertices[k]) == len(verts) and tuple(int(v) for v in r.rect[k]) == box
        assert [tuple(int(c) for c in v) for v in r.polygon(k)] == verts[:n] and r.polygon(k).shape == (n, 2)
        assert not r.vertices[k, n:].any(), "the slots behind a row's vertices are 0"


def inside(points, corners, eps=1e-9):
    """every point lies in the rectangle with the given corners (in order; sides may have no length), within eps"""
    c0, u, v = corners[0], corners[1] - corners[0], corners[3] - corners[0]
    rel = points - c0
    back = np.zeros_like(rel)
    for side in (u, v):
        length = np.hypot(*side)
        if length > 0:
            t = rel @ side / length                       # along the side, in pixels
            assert t.min() >= -eps and t.max() <= length + eps, (t.min(), t.max(), length)
            back += np.outer(t / length, side)
    assert np.abs(rel - back).max() <= eps, "off the rectangle's plane part"


@both_backends
def test_numpy_torch_and_gap(backend):
    text, exp, _, exp_geo = case("noise0.35", 40, 50, 8, 3)
    mask = (text != 0).astype(np.uint8) * 255
    keep = mask.copy()
    with BACKENDS[backend]() as dev:
        r = T.region_geometry(mask, min_area=3, max_vertices=16, device=dev)
        t_in = torch.from_numpy(mask).to(dev)
        rt = T.region_geometry(t_in, connectivity=8, min_area=3, max_regions=4, max_vertices=3, device=dev)
        assert torch.equal(t_in.cpu(), torch.from_numpy(keep)), "the argument must not be modified"
        assert isinstance(rt.regions.labels, torch.Tensor) and rt.regions.labels.device == t_in.device
        rt_labels = rt.regions.labels.cpu().numpy()
        rb = T.region_geometry(mask, min_area=3, gap=2, device=dev)
        blocks = T.text_blocks(mask, 2, min_area=3, device=dev)
    assert np.array_equal(mask, keep)
    assert isinstance(r, T.RegionGeometry) and isinstance(r.regions, T.TextRegions) and isinstance(r.regions.labels, np.ndarray)
    assert np.array_equal(r.regions.labels, exp["labels"]) and np.array_equal(r.regions.table, exp["table"])
    assert (r.regions.found, r.regions.kept, r.regions.truncated) == (*exp["n"], False)
    check_against(r, exp, exp_geo, 16)
    assert rt.regions.truncated and np.array_equal(rt.regions.table, exp["table"][:4]) and np.array_equal(rt_labels, exp["labels"])
    check_against(rt, exp, exp_geo, 3, rows=4)
    assert isinstance(rb.regions, T.TextBlocks) and np.array_equal(rb.regions.labels, blocks.labels) and np.array_equal(rb.regions.table, blocks.table)
    assert np.array_equal(rb.regions.members, blocks.members) and rb.regions.kept == blocks.kept < exp["n"][1] and np.array_equal(rb.regions.mask, blocks.mask)
    check_against(rb, None, expected_geometry(blocks.labels, blocks.table, len(blocks.table)), 64)


@both_backends
@pytest.mark.parametrize("name,h,w", PATTERNS, ids=[p[0] for p in PATTERNS])
def test_helpers(backend, name, h, w):
    text, exp, _, exp_geo = case(name, h, w)
    with BACKENDS[backend]() as dev:
        r = T.region_geometry(text, device=dev)
    check_against(r, exp, exp_geo, 64)
    square = np.array([[-0.5, -0.5], [-0.5, 0.5], [0.5, 0.5], [0.5, -0.5]])
    for k, (verts, box) in enumerate(exp_geo):
        ys, xs = np.nonzero(exp["labels"] == exp["table"][k][0])
        pts = np.stack([ys, xs], axis=1).astype(np.float64)
        corners, padded = r.box_points(k), r.box_points(k, pad=True)
        assert corners.shape == (4, 2) and corners.dtype == np.float64
        inside(pts, corners)
        inside((pts[:, None, :] + square[None]).reshape(-1, 2), padded)
        _, dy, dx, lo_d, hi_d, lo_n, hi_n, dd = box
        along, across = r.size(k)
        assert abs(along * across - (hi_d - lo_d) * (hi_n - lo_n) / dd) <= 1e-9 * max(1.0, along * across)
        assert abs(along - np.hypot(*(corners[1] - corners[0]))) <= 1e-9 and abs(across - np.hypot(*(corners[3] - corners[0]))) <= 1e-9
        grow = (abs(dy) + abs(dx)) / np.sqrt(dd)
        assert np.allclose(r.size(k, pad=True), (along + grow, across + grow), rtol=0, atol=1e-9)
        assert -90.0 < r.angle(k) <= 90.0
        if len(verts) == 1:
            assert np.array_equal(corners, np.tile(pts[0], (4, 1))) and (along, across) == (0.0, 0.0) and r.angle(k) == 0.0
    if name in ("row", "box"):
        assert r.angle(0) == 0.0
    if name == "column":
        assert r.angle(0) == 90.0
    if name == "diagonal":
        assert r.angle(0) == 45.0


@both_backends
def test_angle_of_the_tilted_rectangle(backend):
    """within one degree of the direction of the longest edge of the rasterised hull, computed here from the restatement's vertices"""
    text, exp, _, exp_geo = case("tilted", 150, 217)
    verts = exp_geo[0][0]
    edges = [(by - ay, bx - ax) for (ay, ax), (by, bx) in zip(verts, verts[1:] + verts[:1])]
    dy, dx = max(edges, key=lambda e: e[0] ** 2 + e[1] ** 2)
    want = np.degrees(np.arctan2(dy, dx))
    want = want - 180.0 if want > 90.0 else want + 180.0 if want <= -90.0 else want
    with BACKENDS[backend]() as dev:
        r = T.region_geometry(text, device=dev)
    assert abs(want - 30.0) < 2.0, "the pattern is turned by 30 degrees towards +y"
    assert abs(r.angle(0) - want) < 1.0, (r.angle(0), want)
    along, across = sorted(r.size(0), reverse=True)
    assert 88.0 < along < 93.0 and 22.0 < across < 27.0, "a 90 x 24 rectangle"


def test_arguments_are_checked():
    mask = np.zeros((4, 4), np.uint8)
    for kw in (dict(connectivity=6), dict(min_area=-1), dict(max_regions=0), dict(max_vertices=2), dict(max_vertices=1025), dict(max_vertices=8.5),
               dict(gap=0), dict(gap=65)):
        with pytest.raises(ValueError):
            T.region_geometry(mask, **kw)
    with pytest.raises(ValueError, match="uint8"):
        T.region_geometry(np.zeros((4, 4), np.float32))
    assert geometry_pattern("pixel", 3, 3).sum() == 1
