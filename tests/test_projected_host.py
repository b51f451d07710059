"""CPU: the projected feature tables' entry points (include/sf_hip.h: sf_projected_*) are exported and bound, reject bad
arguments before touching the device, and the engine's `project` switch and the registry behave -- no GPU here."""
import ctypes as C

import pytest


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from speaker_follower_amd import _lib
    return _lib


NEW = ('sf_projected_ld', 'sf_projected_build', 'sf_projected_register', 'sf_projected_registered', 'sf_projected_use',
       'sf_projected_is_used', 'sf_projected_steps', 'sf_debug_projected_partials_late', 'sf_projected_supported',
       'sf_debug_projected_chunk_rows')


def test_new_symbols_are_exported_and_bound():
    L = _lib()
    raw = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in L.EXPORTS
        assert getattr(L.lib, name).argtypes is not None
    assert L.lib.sf_abi_version() == 10                             # (additive; 10 is the removal of the retired schedules' fields)


def test_row_stride_is_h_plus_one_padded_to_16_bytes():
    L = _lib()
    assert L.lib.sf_projected_ld(512) == 516
    assert L.lib.sf_projected_ld(8) == 12 and L.lib.sf_projected_ld(4) == 8
    assert L.lib.sf_projected_ld(0) == 0 and L.lib.sf_projected_ld(-4) == 0
    for h in (4, 64, 256, 512):
        ld = L.lib.sf_projected_ld(h)
        assert ld % 4 == 0 and h + 1 <= ld < h + 5


def test_struct_layout():
    L = _lib()
    assert C.sizeof(L.Projected) == 7 * 8 + 6 * 4
    assert [n for n, _ in L.Projected._fields_] == ['pv', 'pa', 'lv', 'la', 'loc_table', 'key_v', 'key_a', 'H', 'ld', 'V',
                                                    'IMG', 'LOC', 'reserved']


def test_argument_validation_without_gpu():
    L = _lib()
    lib = L.lib
    fold = L.DecoderFold(1 << 20, 1 << 20, 1 << 20, 1 << 20)
    ok = dict(fold=C.byref(fold), table=1 << 20, n=36, loc=1 << 20, V=36, IMG=2048, LOC=128, H=512)

    def build(**kw):
        a = dict(ok, **kw)
        return lib.sf_projected_build(a['fold'], a['table'], a['n'], a['loc'], a['V'], a['IMG'], a['LOC'], a['H'],
                                      1 << 20, 1 << 20, 1 << 20, 1 << 20, None, 0, None)
    assert build(fold=None) == L.SF_ERR_ARG
    assert build(table=None) == L.SF_ERR_ARG and build(loc=None) == L.SF_ERR_ARG
    assert build(n=0) == L.SF_ERR_ARG and build(V=0) == L.SF_ERR_ARG
    assert build(IMG=2050) == L.SF_ERR_ARG and build(LOC=120) == L.SF_ERR_ARG and build(H=510) == L.SF_ERR_ARG
    assert lib.sf_projected_build(C.byref(L.DecoderFold()), 1 << 20, 36, 1 << 20, 36, 2048, 128, 512, 1 << 20, 1 << 20,
                                  1 << 20, 1 << 20, None, 0, None) == L.SF_ERR_ARG
    assert build() == L.SF_ERR_WORKSPACE                            # (every argument fine: stops at the missing workspace)
    # a table registered as binary16 has no fp32 rows to project
    assert lib.sf_feature_table_f16(C.c_void_p(1 << 21), 1) == 0
    try:
        assert build(table=1 << 21) == L.SF_ERR_UNSUPPORTED
    finally:
        lib.sf_feature_table_f16(C.c_void_p(1 << 21), 0)


def test_registry_keeps_one_entry_per_table_address():
    L = _lib()
    lib = L.lib
    t1, t2 = C.c_void_p(0x1000), C.c_void_p(0x2000)
    good = L.Projected(0x10, 0x20, 0x30, 0x40, 0x50, 0x60, 0x70, 512, 516, 36, 2048, 128, 0)
    assert lib.sf_projected_register(None, C.byref(good)) == L.SF_ERR_ARG
    for bad in (dict(pv=None), dict(la=None), dict(loc_table=None), dict(key_v=None), dict(H=0), dict(H=510), dict(ld=513),
                dict(V=0), dict(IMG=0), dict(LOC=0)):
        p = L.Projected(0x10, 0x20, 0x30, 0x40, 0x50, 0x60, 0x70, 512, 516, 36, 2048, 128, 0)
        for k, v in bad.items():
            setattr(p, k, v)
        assert lib.sf_projected_register(t1, C.byref(p)) == L.SF_ERR_ARG, bad
    assert lib.sf_projected_registered(t1, None) == 0
    assert lib.sf_projected_register(t1, None) == 0                 # unknown address: nothing to do
    try:
        assert lib.sf_projected_register(t1, C.byref(good)) == 0
        out = L.Projected()
        assert lib.sf_projected_registered(t1, C.byref(out)) == 1 and out.pv == 0x10 and out.key_a == 0x70 and out.ld == 516
        assert lib.sf_projected_registered(t2, None) == 0 and lib.sf_projected_registered(None, None) == 0
        other = L.Projected(0x11, 0x21, 0x31, 0x41, 0x51, 0x61, 0x71, 512, 516, 36, 2048, 128, 0)
        assert lib.sf_projected_register(t1, C.byref(other)) == 0   # the same address again: replaced, not a second entry
        assert lib.sf_projected_registered(t1, C.byref(out)) == 1 and out.pv == 0x11
        # sixteen addresses fit, the seventeenth is refused
        extra = [C.c_void_p(0x100000 + 0x1000 * i) for i in range(16)]
        codes = [lib.sf_projected_register(a, C.byref(good)) for a in extra]
        assert codes == [0] * 15 + [L.SF_ERR_UNSUPPORTED]
        for a in extra:
            lib.sf_projected_register(a, None)
    finally:
        lib.sf_projected_register(t1, None)
    assert lib.sf_projected_registered(t1, None) == 0


def test_use_switch_and_step_counter():
    L = _lib()
    from speaker_follower_amd import follower
    assert L.lib.sf_projected_is_used() == 1                        # default: on
    steps0 = L.lib.sf_projected_steps()
    assert steps0 >= 0
    with follower.projected_pass(False):
        assert L.lib.sf_projected_is_used() == 0
        with follower.projected_pass(True):
            assert L.lib.sf_projected_is_used() == 1
        assert L.lib.sf_projected_is_used() == 0
    assert L.lib.sf_projected_is_used() == 1
    assert L.lib.sf_projected_steps() == steps0                     # toggling the switch issues nothing


def test_engine_switch_values():
    from speaker_follower_amd import follower
    eng = follower.FollowerEngine(None, None, None)
    assert eng.project == 'auto'
    for ok in (True, False, 'auto'):
        eng.project = ok
        assert eng.project is ok or eng.project == ok
    for bad in ('on', 1, 0, None, 'true'):
        with pytest.raises(ValueError):
            eng.project = bad
    eng.project = False
    assert eng._projected_tables(16) is None                        # never asks the store
    eng.project = True
    assert eng._projected_tables(follower.PROJECT_MAX_B + 1) is None


def test_supported_query_follows_the_chain_limits():
    """What the engine asks before it builds anything: the shape limits of the chain (csrc/sf_attention.hip:
    proj_chain_supported), without a device."""
    L = _lib()
    q = L.lib.sf_projected_supported
    ok = dict(B=100, H=512, L=80, A=14, V=36, IMG=2048, LOC=128)
    assert q(*ok.values()) == 1
    for bad in (dict(B=257), dict(B=0), dict(H=516), dict(H=510), dict(H=0), dict(L=0), dict(L=161), dict(A=17), dict(A=0),
                dict(V=18), dict(V=37), dict(IMG=2050), dict(LOC=120), dict(IMG=4096)):
        assert q(*dict(ok, **bad).values()) == 0, bad
    for fine in (dict(B=1), dict(B=256), dict(A=16), dict(A=1), dict(L=160), dict(V=19), dict(H=256)):
        assert q(*dict(ok, **fine).values()) == 1, fine


def test_engine_asks_the_library_before_it_touches_the_store():
    """A shape the chain declines (17 candidate slots) or a store it cannot read (fp16): no table lookup, no build, no mark."""
    from speaker_follower_amd import follower

    class Store:
        dtype, V, IMG, LOC = 'fp32', 36, 2048, 128
        def projected(self, *a, **k): raise AssertionError('the store was asked')
        def note_unprojected(self, *a): raise AssertionError('the pair was marked')
        def seen_unprojected(self, *a): return False

    class Dec:
        hidden_size = 512
    for mode in ('auto', True):
        eng = follower.FollowerEngine(None, Dec(), Store())
        eng.project = mode
        assert eng._projected_tables(16, T=20, A=17) is None
        eng.store.dtype = 'fp16'
        assert eng._projected_tables(16, T=20, A=14) is None
        Store.dtype = 'fp32'
