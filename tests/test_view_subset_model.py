"""The model of the view list (tests/view_subset_model.py) on named hand cases, written out by hand: what the header of
include/fasterhip_view_subset.h promises, and for every deliberate mistake of the model a case that it changes — a test against the
model can tell each of them from the truth.  No GPU."""
import numpy as np
import pytest

import view_subset_model as vm

# name: (active, view_of, n, n_views, the list by hand, the count by hand)
CASES = {
    "fewer queries than views": (None, None, 2, 5, [0, 1, -1, -1, -1], 2),
    "some inactive": ([1, 0, 0, 1, 1], None, 5, 5, [0, 3, 4, -1, -1], 3),
    "nobody active": ([0, 0, 0], None, 3, 3, [-1, -1, -1], 0),
    "active is any non-zero word": ([7, 0, -1], None, 3, 3, [0, 2, -1], 2),
    "teams": (None, [2, 2, 0, 0, 2, 0], 6, 3, [0, 2, -1], 2),
    "teams in descending order": (None, [3, 1, 3, 0], 4, 4, [0, 1, 3, -1], 3),
    "a team goes when all of it is inactive": ([1, 0, 0, 0, 1, 0], [0, 1, 1, 1, 2, 0], 6, 3, [0, 2, -1], 2),
    "views outside the range": (None, [-1, 4, 1, 1 << 30, -(1 << 31)], 5, 4, [1, -1, -1, -1], 1),
    "an inactive query with a view outside": ([0, 1], [9, 0], 2, 2, [0, -1], 1),
    "one view": ([1, 1, 1], [0, 0, 0], 3, 1, [0], 1),
    "one view, nobody": ([0], None, 1, 1, [-1], 0),
    "no query": (None, None, 0, 3, [-1, -1, -1], 0),
    "every view needed leaves no tail": (None, [1, 0, 1, 0], 4, 2, [0, 1], 2),
}
# variant: the cases it must change
CHANGED_BY = {
    "active_ignored": ("some inactive", "nobody active", "a team goes when all of it is inactive", "one view, nobody"),
    "out_of_range_kept": ("views outside the range",),
    "duplicates_kept": ("teams", "one view"),
    "tail_zero": ("fewer queries than views", "nobody active", "no query"),
    "first_appearance": ("teams", "teams in descending order"),
}


def _run(name, variant=None):
    active, view_of, n, n_views, _, _ = CASES[name]
    return vm.view_list(None if active is None else np.array(active, dtype=np.int32), None if view_of is None else np.array(view_of, dtype=np.int64),
                        n, n_views, variant)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_case(name):
    got, count = _run(name)
    want, want_count = CASES[name][4:]
    assert got.dtype == np.int32 and got.tolist() == want and count == want_count
    # the promises of the header: ascending, each once, -1 behind, as many entries as views
    assert len(got) == CASES[name][3] and (np.diff(got[:count]) > 0).all() and (got[count:] == -1).all()


@pytest.mark.parametrize("variant", vm.VARIANTS)
def test_every_wrong_variant_changes_its_cases(variant):
    for name in CHANGED_BY[variant]:
        got, count = _run(name, variant)
        assert (got.tolist(), count) != (CASES[name][4], CASES[name][5]), (variant, name)


def test_every_case_is_changed_by_some_variant():
    changed = {name for name in CASES for v in vm.VARIANTS if (_run(name, v)[0].tolist(), _run(name, v)[1]) != (CASES[name][4], CASES[name][5])}
    assert changed == set(CASES)
    assert set(CHANGED_BY) == set(vm.VARIANTS)


def test_listed_reads_what_a_listed_read_reads():
    assert vm.listed([3, -1, 70, 3, 5, 6], 4, 70) == {3}
    assert vm.listed([0, 1, 2], 9, 3) == {0, 1, 2} and vm.listed([0, 1, 2], 0, 3) == set() and vm.listed([0, 1, 2], -4, 3) == set()
