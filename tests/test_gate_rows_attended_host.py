"""CPU: gate-space rows for the ATTENDED half of the decoder LSTM's input (include/sf_hip.h: sf_gate_rows_attended_*).
The entry points are declared, exported and bound without an ABI bump and reject bad arguments before touching the device;
the registry and the switch behave; and the algebra the table rests on -- which columns of W_ih it multiplies, how its rows
are laid out, which columns are left to the short product -- is held to a float64 numpy product on a tiny case.  No GPU."""
import ctypes as C
import os

import numpy as np


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from speaker_follower_amd import _lib
    return _lib


NEW = ('sf_gate_rows_attended_build', 'sf_gate_rows_attended_register', 'sf_gate_rows_attended_registered',
       'sf_gate_rows_attended_use', 'sf_gate_rows_attended_is_used', 'sf_gate_rows_attended_steps',
       'sf_gate_rows_attended_supported', 'sf_lstm_cell_rows_fwd')


def test_abi_stays_10_and_the_new_symbols_are_declared_exported_and_bound():
    L = _lib()
    assert L.ABI_VERSION == 10 and L.lib.sf_abi_version() == 10     # (additive: no existing struct changed)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sf_hip.h')).read()
    raw = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name + '(' in header, name
        assert hasattr(raw, name), name
        assert name in L.EXPORTS and name in L.HEADER.functions
    # the existing struct is what it was; the new table has a struct of its own
    assert C.sizeof(L.GateRows) == 3 * 8 + 4 * 4
    assert [n for n, _ in L.GateRows._fields_] == ['gu', 'gl', 'key_w', 'H', 'V', 'IMG', 'LOC']
    assert C.sizeof(L.GateRowsAttended) == 2 * 8 + 4 * 4
    assert [n for n, _ in L.GateRowsAttended._fields_] == ['gf', 'key_w', 'H', 'V', 'IMG', 'LOC']


def test_argument_validation_without_gpu():
    L = _lib()
    lib = L.lib
    ok = dict(w=1 << 20, table=1 << 20, n=36, IMG=2048, LOC=128, H=512, gf=1 << 20)

    def build(**kw):
        a = dict(ok, **kw)
        return lib.sf_gate_rows_attended_build(a['w'], a['table'], a['n'], a['IMG'], a['LOC'], a['H'], a['gf'], None, 0, None)
    for bad in (dict(w=None), dict(table=None), dict(gf=None), dict(n=0), dict(IMG=2050), dict(IMG=0), dict(LOC=120),
                dict(LOC=0), dict(H=510), dict(H=0)):
        assert build(**bad) == L.SF_ERR_ARG, bad
    assert lib.sf_feature_table_f16(C.c_void_p(1 << 21), 1) == 0    # a binary16 table has no fp32 rows to carry over
    try:
        assert build(table=1 << 21) == L.SF_ERR_UNSUPPORTED
    finally:
        lib.sf_feature_table_f16(C.c_void_p(1 << 21), 0)
    # the cell alone: a row and a column range are required, the path is 0, 1 or 2
    w = L.LstmW(1 << 20, 1 << 20, 1 << 20, 1 << 20)
    p = 1 << 20

    def cell(x_col0=2176, xg=p, path=0, I=4352):
        return lib.sf_lstm_cell_rows_fwd(C.byref(w), 4, I, 512, p, I, x_col0, xg, None, p, p, p, p, None, path, None, 0, None)
    for bad in (dict(xg=None), dict(x_col0=0), dict(x_col0=4352), dict(x_col0=2178), dict(path=3), dict(path=-1)):
        assert cell(**bad) == L.SF_ERR_ARG, bad


def test_supported_is_the_partials_rule_on_rows_of_4h_plus_loc_floats():
    """H <= 512 at LOC = 128: ceil(H / 64) image slots and one location slot within the nine a lane holds; and what is left
    of the product, LOC + H, is a short reduction."""
    lib = _lib().lib
    assert [H for H in (64, 128, 256, 384, 512, 576, 640, 1024) if lib.sf_gate_rows_attended_supported(H, 128)] == \
        [64, 128, 256, 384, 512]
    assert lib.sf_gate_rows_attended_supported(512, 256) == 1 and lib.sf_gate_rows_attended_supported(512, 260) == 0
    assert lib.sf_gate_rows_attended_supported(0, 128) == 0 and lib.sf_gate_rows_attended_supported(512, 0) == 0
    assert lib.sf_gate_rows_attended_supported(510, 128) == 0


def test_registry_and_switch():
    L = _lib()
    lib = L.lib
    from speaker_follower_amd import follower
    t1 = C.c_void_p(0x5000)
    good = L.GateRowsAttended(0x10, 0x30, 512, 36, 2048, 128)
    assert lib.sf_gate_rows_attended_register(None, C.byref(good)) == L.SF_ERR_ARG
    for bad in (dict(gf=None), dict(key_w=None), dict(H=0), dict(H=510), dict(V=0), dict(IMG=0), dict(LOC=0)):
        g = L.GateRowsAttended(0x10, 0x30, 512, 36, 2048, 128)
        for k, v in bad.items():
            setattr(g, k, v)
        assert lib.sf_gate_rows_attended_register(t1, C.byref(g)) == L.SF_ERR_ARG, bad
    assert lib.sf_gate_rows_attended_registered(t1, None) == 0
    try:
        assert lib.sf_gate_rows_attended_register(t1, C.byref(good)) == 0
        out = L.GateRowsAttended()
        assert lib.sf_gate_rows_attended_registered(t1, C.byref(out)) == 1 and out.gf == 0x10 and out.key_w == 0x30
        assert lib.sf_gate_rows_registered(t1, None) == 0           # (a registry of its own)
    finally:
        lib.sf_gate_rows_attended_register(t1, None)
    assert lib.sf_gate_rows_attended_registered(t1, None) == 0
    assert lib.sf_gate_rows_attended_is_used() == 1                 # default: on
    steps0 = lib.sf_gate_rows_attended_steps()
    with follower.gate_rows_attended_pass(False):
        assert lib.sf_gate_rows_attended_is_used() == 0 and lib.sf_gate_rows_is_used() == 1
        with follower.gate_rows_attended_pass(True):
            assert lib.sf_gate_rows_attended_is_used() == 1
        assert lib.sf_gate_rows_attended_is_used() == 0
    assert lib.sf_gate_rows_attended_is_used() == 1 and lib.sf_gate_rows_attended_steps() == steps0


def test_engine_switch_defaults_on_and_reaches_the_store_only_when_off():
    from speaker_follower_amd import follower

    class Store:
        asked = []
        def gate_rows(self, decoder, build=True, **kw):
            self.asked.append(kw)
            return 'rows'

    eng = follower.FollowerEngine(None, None, Store())
    assert eng.gate_rows_attended is True
    assert eng._gate_rows_tables({'bufs': ()}, False) == 'rows' and Store.asked == [{}]
    eng.gate_rows_attended = False
    assert eng._gate_rows_tables({'bufs': ()}, False) == 'rows' and Store.asked == [{}, {'attended': False}]
    eng.gate_rows = False                                           # (means something only while gate_rows is on)
    eng.gate_rows_attended = True
    assert eng._gate_rows_tables({'bufs': ()}, False) is None and len(Store.asked) == 2


def test_table_layout_and_the_columns_of_w_ih_against_float64():
    """A tiny decode step in float64.  The LSTM input is [u | f] with f = sum_v alpha_v [table[vp, v] | loc[view, v]]:
        gates_x = u W[:, :F]^T + f_img W[:, F:F+IMG]^T + f_loc W[:, F+IMG:2F]^T.
    The table holds row (vp V + v) = table[vp, v] W[:, F:F+IMG]^T, so the middle term is sum_v alpha_v GF[vp V + v] -- the
    IMAGE columns [F, F+IMG) of the attended half and no others -- and the short product that remains runs over the
    LOCATION columns [F+IMG, 2F) of both xin and W_ih (leading dimension 2F)."""
    rng = np.random.default_rng(7)
    n_vp, V, IMG, LOC, H, B = 3, 5, 8, 4, 6, 4
    F, N = IMG + LOC, 4 * H
    table = rng.standard_normal((n_vp, V, IMG))
    loc = rng.standard_normal((V, V, LOC))
    w = rng.standard_normal((N, 2 * F))
    vp, view = np.array([0, 2, 1, 2]), np.array([4, 0, 3, 1])
    alpha = rng.random((B, V))
    alpha /= alpha.sum(axis=1, keepdims=True)
    u = rng.standard_normal((B, F))
    f = np.einsum('bv,bvk->bk', alpha, np.concatenate([table[vp], loc[view]], axis=2))
    want = np.concatenate([u, f], axis=1) @ w.T
    # the table: [n_vp * V, 4H], row-major over (viewpoint, view), against the image columns of the attended half
    gf = table.reshape(n_vp * V, IMG) @ w[:, F:F + IMG].T
    assert gf.shape == (n_vp * V, N)
    rows = vp[:, None] * V + np.arange(V)[None, :]
    xg_f = np.einsum('bv,bvn->bn', alpha, gf[rows])
    xin = np.concatenate([u, f], axis=1)
    short = xin[:, F + IMG:2 * F] @ w[:, F + IMG:2 * F].T           # {xin + F + IMG, 2F, W_ih + F + IMG, 2F, LOC}
    got = u @ w[:, :F].T + xg_f + short
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # the image part alone is what the table replaces, the location part alone what the short product keeps
    assert np.abs(xg_f - f[:, :IMG] @ w[:, F:F + IMG].T).max() <= 1e-12 * np.abs(xg_f).max()
    assert np.abs(short - f[:, IMG:] @ w[:, F + IMG:].T).max() <= 1e-12 * np.abs(short).max()
    # ... and NOT the action half's image columns [0, IMG), which gu holds: the two tables differ
    assert np.abs(table.reshape(-1, IMG) @ w[:, :IMG].T - gf).max() > 1e-3 * np.abs(gf).max()
