"""CPU: how many text groups per sample launch (1) of the projected decode chain runs (include/sf_hip.h:
sf_projected_text_groups_plan; csrc/sf_attention.hip: proj_text_groups_plan, the function the launcher itself calls).

The rule: two groups iff the attention partials ride in the launch, L <= 80 and the four-group grid 3 B + 4 B + product
blocks exceeds the workgroups the device holds at once.  Checked at 512 slots (256 CUs x 2 workgroups) and the 32 product
blocks of y at H = 512 -- no GPU here."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS, NA = 512, 32


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from speaker_follower_amd import _lib
    return _lib


def _plan(B, L, partials=1, slots=SLOTS, na=NA):
    grid = C.c_int(-1)
    g = _lib().lib.sf_projected_text_groups_plan(B, L, partials, slots, na, C.byref(grid))
    return g, grid.value


def test_first_batch_over_the_slots():
    assert 7 * 68 + NA == 508 and 7 * 69 + NA == 515
    assert _plan(68, 80) == (4, 508)                                # fits: nothing changes
    assert _plan(69, 80) == (2, 3 * 69 + 2 * 69 + NA)               # the first batch whose four-group grid does not
    assert _plan(69, 80)[1] == 377


def test_headline_batch():
    assert _plan(100, 80) == (2, 532)
    assert _plan(100, 1) == (2, 532)                                # (the rule looks at L only for the ladder's limit)


def test_length_limit_of_the_two_group_ladder():
    assert _plan(100, 80) == (2, 532)
    assert _plan(100, 81) == (4, 732)
    assert _plan(100, 160) == (4, 732)


def test_without_partials_four_groups():
    assert _plan(100, 80, partials=0) == (4, 4 * 100 + NA)
    assert _plan(256, 20, partials=0) == (4, 4 * 256 + NA)


def test_batch_edges():
    assert _plan(1, 80) == (4, 7 + NA)
    assert _plan(256, 80) == (2, 5 * 256 + NA)


def test_unknown_slots_keep_four_groups_and_bad_arguments_are_refused():
    assert _plan(100, 80, slots=0) == (4, 732)
    lib = _lib().lib
    for bad in ((0, 80, 1, SLOTS, NA), (100, 0, 1, SLOTS, NA), (100, 80, 1, -1, NA), (100, 80, 1, SLOTS, -1)):
        assert lib.sf_projected_text_groups_plan(*bad, None) == 0, bad
    assert lib.sf_projected_text_groups_plan(100, 80, 1, SLOTS, NA, None) == 2      # (the grid is optional)


def test_rule_is_monotonic_in_the_batch():
    """Below the first crowded batch always four, from it on always two: one threshold per (L, slots)."""
    groups = [_plan(B, 40)[0] for B in range(1, 257)]
    first = groups.index(2)
    assert first + 1 == 69 and set(groups[:first]) == {4} and set(groups[first:]) == {2}


def test_switch_does_not_reach_the_pure_query():
    lib = _lib().lib
    try:
        for force in (2, 4, 0, 3):
            lib.sf_debug_projected_text_groups(force)
            assert _plan(16, 80) == (4, 7 * 16 + NA) and _plan(100, 80) == (2, 532)
    finally:
        lib.sf_debug_projected_text_groups(0)


def test_abi_version_and_new_symbols():
    L = _lib()
    raw = C.CDLL(L.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'sf_hip.h')).read()
    for name in ('sf_debug_projected_text_groups', 'sf_projected_text_groups_plan'):
        assert hasattr(raw, name), name
        assert name in L.EXPORTS
        assert getattr(L.lib, name).argtypes is not None
        assert name + '(' in header
    assert L.lib.sf_abi_version() == 10 and L.ABI_VERSION == 10     # (additive; 10 is the removal of the retired schedules' fields)
    assert '#define SF_ABI_VERSION 10' in header
