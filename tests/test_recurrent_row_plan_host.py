"""CPU: the pure rules of the recurrent half as a row (include/sf_hip.h: sf_gate_rows_recurrent_use) --
csrc/sf_attention_plan.h: pair_proj_score_hh_accepts (what launch (2) takes of the product's plan) and
csrc/sf_gemm_plan.h: recurrent_row_cell (the shapes of the cell behind it), compiled with g++ through
tests/recurrent_row_plan_shim.cpp; and the library's own entry sf_gate_rows_recurrent_supported, the switch and the
engine attribute, none of which needs a GPU.  Expectations are the rules written down, not read from the headers."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp('recurrent_row_plan') / 'recurrent_row_plan_shim.so'
    subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-shared', '-fPIC',
                    '-I' + os.path.join(ROOT, 'speaker_follower_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'recurrent_row_plan_shim.cpp'), '-o', str(so)], check=True)
    return C.CDLL(str(so))


def test_launch_2_accepts_four_chunks_per_wave_at_one_two_or_four_tile_rows(shim):
    got = {(m, c) for m in range(1, 9) for c in (1, 2, 4, 8, 16, 18) if shim.shim_hh_accepts(m, c)}
    assert got == {(1, 4), (2, 4), (4, 4)}


def _plan(shim, B, H):
    mt, cpw = C.c_int(-1), C.c_int(-1)
    ok = shim.shim_small_shape(B, 4 * H, (H + 15) // 16, C.byref(mt), C.byref(cpw))
    return ok, mt.value, cpw.value


def test_the_product_plan_over_a_sweep_of_batches_and_widths(shim):
    """[B, H] x [4H, H]^T: chunks = ceil(H / 16) over 8 waves.  At H = 512 (32 chunks, four per wave) every batch the
    projected chain takes (B <= 256) plans an accepted (mt, 4); the tile rows per block follow small_shape's coverage rule
    (tile rows per block halved while 128 n-tiles x the blocks of tile rows stay below 224): one up to 32 rows, two up to
    64 (three tile rows round down to two), four from 65 on."""
    for B in (1, 16, 17, 32):
        assert _plan(shim, B, 512) == (1, 1, 4), B
    for B in (33, 48, 49, 64):
        assert _plan(shim, B, 512) == (1, 2, 4), B
    for B in (65, 100, 128, 256):
        assert _plan(shim, B, 512) == (1, 4, 4), B
    assert _plan(shim, 100, 512)[1:] == (4, 4)                      # the headline: a 128 x 2 grid of product blocks
    # narrower decoders: two chunks per wave or fewer -- cpw 2, which launch (2) has no body for: the row is not formed
    for H in (32, 64, 128, 256):
        ok, mt, cpw = _plan(shim, 100, H)
        assert ok and cpw == 2 and not shim.shim_hh_accepts(mt, cpw), H
    for H in (264, 384, 500, 512):                                  # 17 .. 32 chunks: cpw 4
        ok, mt, cpw = _plan(shim, 100, H)
        assert ok and cpw == 4 and shim.shim_hh_accepts(mt, cpw), H
    ok, mt, cpw = _plan(shim, 100, 520)                             # 33 chunks: five per wave
    assert ok and cpw == 8 and not shim.shim_hh_accepts(mt, cpw)


def test_cell_shape_rule_over_a_sweep(shim):
    """recurrent_row_cell(K_x, H): 0 < K_x <= 256, K_x % 4 == 0, H > 0, H % 8 == 0 -- H need NOT be a multiple of 16 (the
    patch is 8 units wide), and nothing left of the product (K_x = 0) is no cell of this kind."""
    for H in (8, 24, 32, 40, 504, 512, 520, 1024):
        for K in (4, 16, 20, 128, 252, 256):
            assert shim.shim_recurrent_row_cell(K, H) == 1, (K, H)
    for H in (0, -8, 4, 12, 510, 513):
        assert shim.shim_recurrent_row_cell(128, H) == 0, H
    for K in (0, -4, 2, 130, 260, 640):
        assert shim.shim_recurrent_row_cell(K, 512) == 0, K


def test_library_entry_switch_and_engine_attribute():
    from speaker_follower_amd import _lib as L, follower
    lib = L.lib
    assert L.ABI_VERSION == 10 and lib.sf_abi_version() == 10       # (additive: no existing struct changed)
    for name in ('sf_gate_rows_recurrent_use', 'sf_gate_rows_recurrent_is_used', 'sf_gate_rows_recurrent_steps',
                 'sf_gate_rows_recurrent_supported', 'sf_lstm_cell_rows3_fwd', 'sf_debug_recurrent_row'):
        assert hasattr(lib, name), name
    # (B, H, LOC) sweep: the attended rows' own rule (H <= 512 at LOC = 128, H % 4, LOC % 4), the cell's, launch (2)'s plan
    assert [B for B in (1, 17, 100, 256) if lib.sf_gate_rows_recurrent_supported(B, 512, 128)] == [1, 17, 100, 256]
    assert lib.sf_gate_rows_recurrent_supported(0, 512, 128) == 0
    assert [H for H in (64, 128, 256, 264, 384, 504, 512, 520, 576)
            if lib.sf_gate_rows_recurrent_supported(100, H, 128)] == [384, 512]    # (H % 16 and H <= 512: the attended rows';
    #                                                                   more than two chunks per wave: launch (2)'s)
    assert lib.sf_gate_rows_recurrent_supported(100, 508, 128) == 0
    assert lib.sf_gate_rows_recurrent_supported(100, 512, 256) == 1
    assert lib.sf_gate_rows_recurrent_supported(100, 512, 0) == 0 and lib.sf_gate_rows_recurrent_supported(100, 512, 130) == 0
    assert lib.sf_gate_rows_recurrent_is_used() == 1                 # default: on
    steps0 = lib.sf_gate_rows_recurrent_steps()
    with follower.gate_rows_recurrent_pass(False):
        assert lib.sf_gate_rows_recurrent_is_used() == 0 and lib.sf_gate_rows_attended_is_used() == 1
        with follower.gate_rows_recurrent_pass(True):
            assert lib.sf_gate_rows_recurrent_is_used() == 1
        assert lib.sf_gate_rows_recurrent_is_used() == 0
    assert lib.sf_gate_rows_recurrent_is_used() == 1 and lib.sf_gate_rows_recurrent_steps() == steps0
    # the entries refuse bad arguments before touching a device
    w = L.LstmW(0x10, 0x20, 0x30, 0x40)
    p = C.c_void_p(0x100)
    assert lib.sf_lstm_cell_rows3_fwd(C.byref(w), 4, 4352, 512, p, 4352, 4224, p, p, None, p, p, p, p, None, None, 0,
                                      None) == L.SF_ERR_ARG
    assert lib.sf_lstm_cell_rows3_fwd(C.byref(w), 4, 4352, 512, p, 4352, 0, p, p, p, p, p, p, p, None, None, 0,
                                      None) == L.SF_ERR_ARG
    assert lib.sf_debug_recurrent_row(C.byref(w), 0, 512, p, 512, p, None) == L.SF_ERR_ARG
    assert lib.sf_debug_recurrent_row(C.byref(w), 4, 512, p, 510, p, None) == L.SF_ERR_ARG


def test_engine_default_is_on():
    from speaker_follower_amd import follower
    eng = follower.FollowerEngine(None, None, None)
    assert eng.gate_rows_recurrent is True and eng.gate_rows_attended is True
