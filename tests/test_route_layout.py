"""``regions.RouteLayout`` and ``regions.unpack_routes``: the one owner of the word offsets of the tensor the flat, smooth and tone stages
leave for ``TextEraser``'s read-back, ``[core counts | found, kept | table | flat rows | smooth rows | tone rows]`` with 6 words per
table row and 5, 5 and 6 per stage row.  Host arrays only: no device, no library.  Every combination of the three stages, with and
without core counts in front, with a table that is cut at ``max_regions`` and one that is not; what is planted at offsets written out
here by hand has to come back, and nothing else: every other word holds a canary.

``regions.ReadBack`` below: the same for the whole tensor of the page's one synchronisation, which puts the first labelling's tensor with
its hull areas, the second labelling's behind ``hull`` and the members and component count of ``group`` around those rows."""
import itertools

import numpy as np
import pytest

from text_segmentation_image_inpainting_amd.regions import RouteLayout, unpack_routes

CANARY = -0x5A5A5A5B
WORDS = {"flat": 5, "smooth": 5, "tone": 6}
CASES = [(f, s, t, nt, n, kept) for (f, s, t), nt, n in itertools.product(itertools.product((False, True), repeat=3), (0, 6), (1, 5))
         for kept in (n - 1, n + 3)]


def _planted(nt, n, kept, enabled, rng):
    """(the array, what is in it) with the offsets spelt out: nt | 2 | 6 n | the enabled stages' rows in the order flat, smooth, tone"""
    rows_in_use = min(kept, n)
    own = np.full(nt + 2 + 6 * n + sum(WORDS[name] * n for name in enabled), CANARY, np.int32)
    counts = rng.integers(0, 1000, nt).astype(np.int32)
    own[:nt] = counts
    own[nt], own[nt + 1] = kept + 4, kept
    table = rng.integers(1, 10000, (rows_in_use, 6)).astype(np.int32)
    own[nt + 2:nt + 2 + 6 * rows_in_use] = table.ravel()
    at, stage_rows = nt + 2 + 6 * n, {}
    for name in enabled:
        rows = rng.integers(0, 256, (rows_in_use, WORDS[name])).astype(np.int32)
        rows[:, 0] = rng.integers(0, 2, rows_in_use)
        own[at:at + WORDS[name] * rows_in_use] = rows.ravel()
        stage_rows[name] = rows
        at += WORDS[name] * n
    return own, counts, table, stage_rows


@pytest.mark.parametrize("flat,smooth,tone,nt,n,kept", CASES)
def test_layout_and_unpack(flat, smooth, tone, nt, n, kept):
    enabled = [name for name, on in (("flat", flat), ("smooth", smooth), ("tone", tone)) if on]
    lay = RouteLayout(nt, n, flat, smooth, tone)
    own, counts, table, stage_rows = _planted(nt, n, kept, enabled, np.random.default_rng(nt + 10 * n + 100 * kept))

    assert lay.words == len(own) and lay.tail == len(own) - (nt + 2 + 6 * n)
    assert lay.stages == tuple(enabled)
    assert (lay.counts, lay.n_regions, lay.table) == (slice(0, nt), slice(nt, nt + 2), slice(nt + 2, nt + 2 + 6 * n))
    at = nt + 2 + 6 * n                                 # the stage slices: in order, disjoint, and the tail exactly
    for name in enabled:
        assert lay.rows(name) == slice(at, at + WORDS[name] * n)
        at = lay.rows(name).stop
    assert at == lay.words
    for name in set(WORDS) - set(enabled):
        with pytest.raises(KeyError):
            lay.rows(name)

    before = own.copy()
    counts_h, got_table, truncated, stages, gone = unpack_routes(own, lay)
    assert np.array_equal(own, before)
    assert np.array_equal(counts_h, counts) and np.array_equal(got_table, table) and got_table.shape == (min(kept, n), 6)
    assert truncated == (kept > n)
    assert list(stages) == enabled
    want_gone = np.zeros(len(table), bool)
    for name in enabled:
        rows, st = stage_rows[name], stages[name]
        assert np.array_equal(st["table"], table)
        assert st["is_" + name].dtype == bool and np.array_equal(st["is_" + name], rows[:, 0] != 0)
        assert st["ring_pixels"].dtype == np.int32 and np.array_equal(st["ring_pixels"], rows[:, 4])
        if name == "flat":
            assert sorted(st) == ["colour", "is_flat", "ring_pixels", "table"]
            assert st["colour"].dtype == np.uint8 and np.array_equal(st["colour"], rows[:, 1:4])
        elif name == "smooth":
            assert sorted(st) == ["is_smooth", "ring_pixels", "step", "table"]
            assert st["step"].dtype == np.uint8 and np.array_equal(st["step"], rows[:, 1:4])
        else:
            assert sorted(st) == ["err", "is_tone", "ring_pixels", "shift", "step", "table"]
            assert np.array_equal(st["shift"], rows[:, 1:3]) and np.array_equal(st["err"], rows[:, 3]) and np.array_equal(st["step"], rows[:, 5])
        want_gone |= rows[:, 0] != 0
    assert gone.dtype == bool and np.array_equal(gone, want_gone)
    for value in [counts_h, got_table, gone] + [v for st in stages.values() for v in st.values()]:
        assert CANARY not in np.asarray(value).astype(np.int64)


# ---- ReadBack: the whole tensor of TextEraser's one synchronisation ------------------------------------------------------------------------
# [first: nt | 2 | 6 n | n hull areas with hull, else the enabled stages' rows]
# [second, with hull and a stage: nt | 2 | 6 n | the enabled stages' rows]
# [with group: n members | the components]
READ_CASES = [(hull, group) + c for hull, group in itertools.product((False, True), repeat=2) for c in CASES]


def _plant_labelling(part, nt, n, kept, rng):
    """fill ``nt | 2 | 6 n`` at the front of ``part`` -> (counts, found, table)"""
    counts = rng.integers(0, 1000, nt).astype(np.int32)
    table = rng.integers(1, 10000, (min(kept, n), 6)).astype(np.int32)
    part[:nt], part[nt], part[nt + 1] = counts, kept + 4, kept
    part[nt + 2:nt + 2 + 6 * len(table)] = table.ravel()
    return counts, kept + 4, table


def _plant_rows(part, at, n, enabled, rows_in_use, rng):
    """the enabled stages' rows from word ``at`` of ``part`` on -> {name: rows}"""
    stage_rows = {}
    for name in enabled:
        rows = rng.integers(0, 256, (rows_in_use, WORDS[name])).astype(np.int32)
        rows[:, 0] = rng.integers(0, 2, rows_in_use)
        part[at:at + WORDS[name] * rows_in_use] = rows.ravel()
        stage_rows[name] = rows
        at += WORDS[name] * n
    return stage_rows


@pytest.mark.parametrize("hull,group,flat,smooth,tone,nt,n,kept", READ_CASES)
def test_read_back_unpack(hull, group, flat, smooth, tone, nt, n, kept):
    import torch
    from text_segmentation_image_inpainting_amd.regions import ReadBack
    enabled = [name for name, on in (("flat", flat), ("smooth", smooth), ("tone", tone)) if on]
    rng = np.random.default_rng(nt + 10 * n + 100 * kept + 1000 * hull + 2000 * group)
    row_words = sum(WORDS[name] * n for name in enabled)
    two = hull and bool(enabled)
    first_words = nt + 2 + 6 * n + (n if hull else row_words)
    second_words = nt + 2 + 6 * n + row_words if two else 0
    host = np.full(first_words + second_words + (n + 1 if group else 0), CANARY, np.int32)

    counts, found, table = _plant_labelling(host, nt, n, kept, rng)
    hull_area = members = components = route_table = gone = None
    stage_rows, plan_counts, plan_table, plan_truncated = {}, counts, table, kept > n
    if hull:
        hull_area = rng.integers(1, 10000, len(table)).astype(np.int32)
        host[nt + 2 + 6 * n:nt + 2 + 6 * n + len(table)] = hull_area
    if two:                                             # the second labelling: its own counts and table, cut when the first is not
        kept2 = n + 3 if kept == n - 1 else n - 1
        second = host[first_words:first_words + second_words]
        plan_counts, _, route_table = _plant_labelling(second, nt, n, kept2, rng)
        stage_rows = _plant_rows(second, nt + 2 + 6 * n, n, enabled, len(route_table), rng)
        plan_truncated = kept2 > n
    elif enabled:
        route_table = table
        stage_rows = _plant_rows(host, nt + 2 + 6 * n, n, enabled, len(table), rng)
    if enabled:
        gone = np.zeros(len(route_table), bool)
        for rows in stage_rows.values():
            gone |= rows[:, 0] != 0
        plan_table = route_table[~gone]
    if group:
        members, components = rng.integers(1, 50, len(table)).astype(np.int32), 77
        host[first_words + second_words:first_words + second_words + len(table)] = members
        host[first_words + second_words + n] = components

    rb = ReadBack(nt, n, hull, group, flat, smooth, tone)
    assert rb.words == len(host) and rb.tail == first_words - (nt + 2 + 6 * n) and rb.second_tail == row_words
    assert rb.n_regions == slice(nt, nt + 2)
    assert rb.routes.words == (second_words if two else nt + 2 + 6 * n + row_words) and rb.routes.stages == tuple(enabled)
    before = host.copy()
    got = rb.unpack(host)
    assert np.array_equal(host, before)
    assert np.array_equal(got.counts, plan_counts) and np.array_equal(got.table, table) and got.table.shape == (min(kept, n), 6)
    assert (got.found, got.kept, got.truncated) == (found, kept, kept > n)
    for value, want in ((got.hull_area, hull_area), (got.members, members), (got.route_table, route_table), (got.gone, gone)):
        assert (value is None and want is None) or (value.dtype == want.dtype and np.array_equal(value, want))
    assert got.components == components
    assert np.array_equal(got.plan_table, plan_table) and got.plan_truncated == plan_truncated
    assert list(got.stages) == enabled
    for name in enabled:
        rows, st = stage_rows[name], got.stages[name]
        assert np.array_equal(st["table"], route_table) and np.array_equal(st["is_" + name], rows[:, 0] != 0)
        assert np.array_equal(st["ring_pixels"], rows[:, 4])
        if name == "tone":
            assert np.array_equal(st["shift"], rows[:, 1:3]) and np.array_equal(st["err"], rows[:, 3]) and np.array_equal(st["step"], rows[:, 5])
        else:
            assert np.array_equal(st["colour" if name == "flat" else "step"], rows[:, 1:4])
    for value in [v for v in got if isinstance(v, np.ndarray)] + [v for st in got.stages.values() for v in st.values()]:
        assert CANARY not in np.asarray(value).astype(np.int64)
    for value in (got.found, got.kept, got.components):
        assert value != CANARY

    # the device side on host tensors: the pieces the stages leave join to exactly this tensor, with a copy only where a piece rides between
    whole_t = torch.from_numpy(np.concatenate([host[:first_words], host[first_words + second_words:]]))
    first_t = whole_t[:first_words]
    second_t = torch.from_numpy(host[first_words:first_words + second_words].copy()) if two else None
    joined = rb.join(first_t, second_t, whole_t if group else None)
    assert np.array_equal(joined.numpy(), host)
    if not two:
        assert joined is (whole_t if group else first_t)


def test_read_back_without_regions():
    from text_segmentation_image_inpainting_amd.regions import ReadBack
    host = np.arange(6, dtype=np.int32)
    rb = ReadBack(6, 5, regions=False)
    got = rb.unpack(host)
    assert rb.words == 6 and got.counts is host and got.stages == {}
    assert all(v is None for v in got._replace(counts=None, stages=None))
