"""The list of needed views (include/fasterhip_view_subset.h, fh_map_view_list_device) restated in numpy, the header's model word for
word: `view_list()` is what the device must write in every byte of d_list and d_count.  `variant` names one deliberate mistake
(tests/test_view_subset_model.py shows which hand case each one changes); None is the model."""
import numpy as np

VARIANTS = ("active_ignored", "out_of_range_kept", "duplicates_kept", "tail_zero", "first_appearance")
POISON = 0x5A


def view_list(active, view_of, n, n_views, variant=None):
    """(d_list [n_views] int32, count).  active: [n] or None (every query), view_of: [n] or None (query q needs view q)."""
    n, n_views = int(n), int(n_views)
    assert n >= 0 and n_views >= 1 and (view_of is not None or n <= n_views)
    needed = []
    for q in range(n):
        if active is not None and int(active[q]) == 0 and variant != "active_ignored":
            continue
        v = int(view_of[q]) if view_of is not None else q
        if not 0 <= v < n_views and variant != "out_of_range_kept":
            continue
        needed.append(v)
    if variant != "duplicates_kept":
        needed = list(dict.fromkeys(needed))   # each once, in the order of first appearance
    if variant != "first_appearance":
        needed = sorted(needed)
    count = len(needed)
    needed = needed[:n_views]   # (only a wrong variant can have more than fit; its count says so)
    out = np.full(n_views, 0 if variant == "tail_zero" else -1, dtype=np.int32)
    out[:len(needed)] = needed
    return out, count


def listed(d_list, count, n_views):
    """The views a listed read rebuilds: the entries below min(count, n_views) that lie in [0, n_views), as a set."""
    return {int(v) for v in np.asarray(d_list)[:max(min(int(count), int(n_views)), 0)] if 0 <= int(v) < int(n_views)}
