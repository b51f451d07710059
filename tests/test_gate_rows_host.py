"""CPU: the gate-space rows' entry points (include/sf_hip.h: sf_gate_rows_*) are declared, exported and bound without an
ABI bump, reject bad arguments before touching the device, the registry and the switches behave, and the location
grouping of `gl` is the one dense candidate rows have -- no GPU here."""
import ctypes as C
import os

import numpy as np


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from speaker_follower_amd import _lib
    return _lib


NEW = ('sf_gate_rows_build', 'sf_gate_rows_register', 'sf_gate_rows_registered', 'sf_gate_rows_use', 'sf_gate_rows_is_used',
       'sf_gate_rows_steps')


def test_abi_stays_10_and_the_new_symbols_are_declared_exported_and_bound():
    L = _lib()
    assert L.ABI_VERSION == 10 and L.lib.sf_abi_version() == 10     # (additive: no existing struct changed)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sf_hip.h')).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name + '(' in header, name
        assert hasattr(raw, name), name
        assert name in L.EXPORTS and name in L.HEADER.functions
        assert getattr(L.lib, name).argtypes is not None
    assert 'sf_gate_rows' in L.STRUCTS


def test_struct_layout():
    L = _lib()
    assert C.sizeof(L.GateRows) == 3 * 8 + 4 * 4
    assert [n for n, _ in L.GateRows._fields_] == ['gu', 'gl', 'key_w', 'H', 'V', 'IMG', 'LOC']


def test_argument_validation_without_gpu():
    L = _lib()
    lib = L.lib
    ok = dict(w=1 << 20, table=1 << 20, n=36, IMG=2048, LOC=128, H=512, gu=1 << 20, gl=1 << 20)

    def build(**kw):
        a = dict(ok, **kw)
        return lib.sf_gate_rows_build(a['w'], a['table'], a['n'], a['IMG'], a['LOC'], a['H'], a['gu'], a['gl'], None, 0, None)
    for bad in (dict(w=None), dict(table=None), dict(gu=None), dict(gl=None), dict(n=0), dict(IMG=2050), dict(IMG=0),
                dict(LOC=120), dict(LOC=0), dict(H=510), dict(H=0)):
        assert build(**bad) == L.SF_ERR_ARG, bad
    assert build() == L.SF_ERR_WORKSPACE                            # (every argument fine: stops at the missing workspace)
    assert lib.sf_feature_table_f16(C.c_void_p(1 << 21), 1) == 0    # a binary16 table has no fp32 rows to carry over
    try:
        assert build(table=1 << 21) == L.SF_ERR_UNSUPPORTED
    finally:
        lib.sf_feature_table_f16(C.c_void_p(1 << 21), 0)


def test_registry_keeps_one_entry_per_table_address():
    L = _lib()
    lib = L.lib
    t1, t2 = C.c_void_p(0x3000), C.c_void_p(0x4000)
    good = L.GateRows(0x10, 0x20, 0x30, 512, 36, 2048, 128)
    assert lib.sf_gate_rows_register(None, C.byref(good)) == L.SF_ERR_ARG
    for bad in (dict(gu=None), dict(gl=None), dict(key_w=None), dict(H=0), dict(H=510), dict(V=0), dict(IMG=0), dict(LOC=0)):
        g = L.GateRows(0x10, 0x20, 0x30, 512, 36, 2048, 128)
        for k, v in bad.items():
            setattr(g, k, v)
        assert lib.sf_gate_rows_register(t1, C.byref(g)) == L.SF_ERR_ARG, bad
    assert lib.sf_gate_rows_registered(t1, None) == 0
    assert lib.sf_gate_rows_register(t1, None) == 0                 # unknown address: nothing to do
    try:
        assert lib.sf_gate_rows_register(t1, C.byref(good)) == 0
        out = L.GateRows()
        assert lib.sf_gate_rows_registered(t1, C.byref(out)) == 1 and out.gu == 0x10 and out.key_w == 0x30 and out.H == 512
        assert lib.sf_gate_rows_registered(t2, None) == 0 and lib.sf_gate_rows_registered(None, None) == 0
        assert lib.sf_projected_registered(t1, None) == 0           # (a registry of its own)
        other = L.GateRows(0x11, 0x21, 0x31, 512, 36, 2048, 128)
        assert lib.sf_gate_rows_register(t1, C.byref(other)) == 0   # the same address again: replaced, not a second entry
        assert lib.sf_gate_rows_registered(t1, C.byref(out)) == 1 and out.gu == 0x11
        extra = [C.c_void_p(0x200000 + 0x1000 * i) for i in range(16)]
        codes = [lib.sf_gate_rows_register(a, C.byref(good)) for a in extra]
        assert codes == [0] * 15 + [L.SF_ERR_UNSUPPORTED]           # sixteen addresses fit, the seventeenth is refused
        for a in extra:
            lib.sf_gate_rows_register(a, None)
    finally:
        lib.sf_gate_rows_register(t1, None)
    assert lib.sf_gate_rows_registered(t1, None) == 0


def test_use_switch_and_step_counter():
    L = _lib()
    from speaker_follower_amd import follower
    assert L.lib.sf_gate_rows_is_used() == 1                        # default: on
    steps0 = L.lib.sf_gate_rows_steps()
    with follower.gate_rows_pass(False):
        assert L.lib.sf_gate_rows_is_used() == 0 and L.lib.sf_projected_is_used() == 1
        with follower.gate_rows_pass(True):
            assert L.lib.sf_gate_rows_is_used() == 1
        assert L.lib.sf_gate_rows_is_used() == 0
    assert L.lib.sf_gate_rows_is_used() == 1
    assert L.lib.sf_gate_rows_steps() == steps0                     # toggling the switch issues nothing


def test_engine_asks_for_gate_rows_only_on_the_projected_chain_and_never_with_bf16_weights():
    from speaker_follower_amd import follower

    class Store:
        asked = []
        def gate_rows(self, decoder, build=True):
            self.asked.append(build)
            return 'rows'

    eng = follower.FollowerEngine(None, None, Store())
    assert eng.gate_rows is True
    assert eng._gate_rows_tables(None, False) is None and Store.asked == []        # no projected tables: not asked
    assert eng._gate_rows_tables({'bufs': ()}, False) == 'rows' and Store.asked == [False]   # 'auto', eager: never builds
    eng._capturing = True
    assert eng._gate_rows_tables({'bufs': ()}, False) == 'rows' and Store.asked == [False, True]
    eng._capturing = False
    eng.project = True
    assert eng._gate_rows_tables({'bufs': ()}, False) == 'rows' and Store.asked == [False, True, True]
    eng.gate_rows = False
    assert eng._gate_rows_tables({'bufs': ()}, False) is None
    eng.gate_rows = True
    eng._gate_weights = 'bf16'
    eng.pass_gate_weights = lambda train=None: 'bf16'              # (an inference pass on packed weights)
    assert eng._gate_rows_tables({'bufs': ()}, False) is None and len(Store.asked) == 3


def test_gl_grouping_matches_float64_on_dense_location_columns():
    """The location part of a DENSE candidate row (the oracle's restatement of the reference's action embedding) times the
    location columns of a weight, in float64, is sum_k sincos_k * gl[k] with gl = features.gate_loc_groups: block k of
    LOC/4 contiguous columns belongs to the k-th of (sin h, cos h, sin e, cos e)."""
    from oracle import np_env
    from speaker_follower_amd import features
    rng = np.random.default_rng(5)
    IMG, LOC, N = 8, 128, 24
    w = rng.standard_normal((N, 2 * (IMG + LOC)))                    # [N, 2F] like W_ih: action half first
    hd, el = np.array([0.0, 0.3, -2.0, 1.1, 3.0]), np.array([0.0, 0.2, -0.4, 0.0, 0.5])
    rows = np_env.action_embedding(rng.standard_normal((36, IMG)).astype(np.float32), [0, 5, 35, 0, 7], hd, el, LOC)
    sc = features.cand_sincos(hd, el).astype(np.float64)
    gl = features.gate_loc_groups(w[:, IMG:IMG + LOC])
    assert gl.shape == (4, N)
    want = rows[1:, IMG:].astype(np.float64) @ w[:, IMG:IMG + LOC].T
    got = sc[1:] @ gl
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # ... and NOT with the values interleaved (column IMG + k, IMG + k + 4, ...): the two layouts differ
    inter = np.stack([w[:, IMG + k:IMG + LOC:4].sum(axis=1) for k in range(4)])
    assert np.abs(sc[1:] @ inter - want).max() > 1e-3 * np.abs(want).max()
    assert np.all(rows[0] == 0)                                     # stop: the zero row, whose gate-space row is zero
