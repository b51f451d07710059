"""CPU: the bidirectional encoder's C entry points (include/sf_hip.h: sf_encoder_bilstm_fwd / sf_encoder_bilstm_bwd) are
exported, bound, and reject null pointers or bad sizes before touching the device; the entries are additive (the ABI version
is the one of the last struct change)."""
import ctypes as C


def _args_fwd(lib_mod, B=4, Lpad=10, T=8, E=300, H=256, nulls=False):
    w = lib_mod.EncoderW()
    tp = lib_mod.EncoderTape(*([64] * 5))
    dev = None if nulls else C.c_void_p(64)            # (never dereferenced: the argument check comes first)
    path = C.c_int32(-7)
    return [None if nulls else C.byref(w), None if nulls else C.byref(w), dev, dev, None, B, Lpad, T, E, H, dev, dev,
            dev, dev, dev, None if nulls else C.byref(tp), None if nulls else C.byref(tp), None, 0, C.byref(path),
            None, 0, None], path


def _args_bwd(lib_mod, B=4, T=8, E=300, H=256, nulls=False):
    w = lib_mod.EncoderW()
    g = lib_mod.EncoderG()
    tp = lib_mod.EncoderTape(*([64] * 5))
    dev = None if nulls else C.c_void_p(64)
    path = C.c_int32(-7)
    return [None if nulls else C.byref(w), None if nulls else C.byref(w), dev, None, C.byref(g), C.byref(g), None, None,
            B, T, E, H, dev, dev, dev, dev, dev, None if nulls else C.byref(tp), None if nulls else C.byref(tp), None, 0,
            C.byref(path), None, 0, None], path


def test_bilstm_entries_are_exported_and_bound():
    from speaker_follower_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ('sf_encoder_bilstm_fwd', 'sf_encoder_bilstm_bwd'):
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS, name
        assert getattr(_lib.lib, name).argtypes is not None, name


def test_bilstm_entries_reject_null_pointers():
    from speaker_follower_amd import _lib
    a, path = _args_fwd(_lib, nulls=True)
    assert _lib.lib.sf_encoder_bilstm_fwd(*a) == 1
    a, path = _args_bwd(_lib, nulls=True)
    assert _lib.lib.sf_encoder_bilstm_bwd(*a) == 1


def test_bilstm_entries_reject_bad_sizes():
    """Valid-looking pointers, then B = 0, T > Lpad, a hidden size no multiple of 16, an embedding width no multiple of
    4: the argument error (1) every time, and the path out-parameter is left alone (nothing ran)."""
    from speaker_follower_amd import _lib
    for kw in (dict(B=0), dict(T=11, Lpad=10), dict(T=0), dict(H=250), dict(E=301)):
        a, path = _args_fwd(_lib, **kw)
        assert _lib.lib.sf_encoder_bilstm_fwd(*a) == 1, kw
        assert path.value == -7, kw
    for kw in (dict(B=0), dict(T=0), dict(H=250), dict(E=301)):
        a, path = _args_bwd(_lib, **kw)
        assert _lib.lib.sf_encoder_bilstm_bwd(*a) == 1, kw
        assert path.value == -7, kw


def test_abi_version_is_still_9():
    from speaker_follower_amd import _lib
    # (10 since the retired schedules' fields left sf_decoder_w and sf_follower_episode; the test keeps its id)
    assert _lib.ABI_VERSION == 10
    assert _lib.lib.sf_abi_version() == 10
