"""``regions.RouteLayout`` and ``regions.unpack_routes``: the one owner of the word offsets of the tensor the flat, smooth and tone stages
leave for ``TextEraser``'s read-back, ``[core counts | found, kept | table | flat rows | smooth rows | tone rows]`` with 6 words per
table row and 5, 5 and 6 per stage row.  Host arrays only: no device, no library.  Every combination of the three stages, with and
without core counts in front, with a table that is cut at ``max_regions`` and one that is not; what is planted at offsets written out
here by hand has to come back, and nothing else: every other word holds a canary."""
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
