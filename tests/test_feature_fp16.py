"""fp16 storage of the feature table, host side: the address registry of the C ABI, the rounding rule of
FeatureStore(dtype='fp16'), and the file format (tsv_to_bin / from_bin).  The device side is tests/test_gpu_feature_fp16.py."""
import base64
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

from speaker_follower_amd import _lib
from speaker_follower_amd.features import FeatureStore, tsv_to_bin

SF_OK, SF_ERR_ARG, SF_ERR_UNSUPPORTED = 0, _lib.SF_ERR_ARG, _lib.SF_ERR_UNSUPPORTED


def _reg(addr, on):
    return _lib.lib.sf_feature_table_f16(C.c_void_p(addr), on)


def _is(addr):
    return _lib.lib.sf_feature_table_is_f16(C.c_void_p(addr))


def test_registry_register_query_forget_full_and_null():
    base = 0x7F0000001000                                  # fake addresses: the registry never dereferences them
    addrs = [base + 64 * i for i in range(17)]
    try:
        assert all(_is(a) == 0 for a in addrs)
        for a in addrs[:16]:
            assert _reg(a, 1) == SF_OK
        assert all(_is(a) == 1 for a in addrs[:16])
        assert _reg(addrs[3], 1) == SF_OK                  # again: still one entry
        assert _reg(addrs[16], 1) == SF_ERR_UNSUPPORTED    # the 17th address is refused ...
        assert _is(addrs[16]) == 0
        assert _reg(addrs[5], 0) == SF_OK                  # ... until one is forgotten
        assert _is(addrs[5]) == 0
        assert _reg(addrs[16], 1) == SF_OK and _is(addrs[16]) == 1
        assert all(_is(a) == 1 for a in addrs[:5] + addrs[6:16])
        assert _reg(addrs[5], 0) == SF_OK                  # unknown address: nothing to do
        assert _lib.lib.sf_feature_table_f16(None, 1) == SF_ERR_ARG
        assert _lib.lib.sf_feature_table_f16(None, 0) == SF_ERR_ARG
        assert _lib.lib.sf_feature_table_is_f16(None) == 0
    finally:
        for a in addrs:
            _reg(a, 0)
    assert all(_is(a) == 0 for a in addrs)
    assert _lib.lib.sf_abi_version() == 10                 # (additive; 10 is the removal of the retired schedules' fields)


def test_fp32_store_clears_a_registered_address_and_fp16_store_registers_its_own():
    t = torch.zeros(2, 3, 8)
    assert _reg(t.data_ptr(), 1) == SF_OK                  # as a collected fp16 table at this address would have left it
    s32 = FeatureStore(t, device='cpu')
    assert s32.table.data_ptr() == t.data_ptr() and s32.dtype == 'fp32'
    assert _is(t.data_ptr()) == 0
    s16 = FeatureStore(t, device='cpu', dtype='fp16')
    addr = s16.table.data_ptr()
    assert s16.dtype == 'fp16' and s16.table.dtype == torch.float16 and _is(addr) == 1
    del s16
    import gc
    gc.collect()
    assert _is(addr) == 0                                  # weakref.finalize forgot it
    with pytest.raises(ValueError):
        FeatureStore(t, device='cpu', dtype='bf16')


def _edge_table():
    """[3, 2, 8]: zero, the fp16 maximum, fp16 subnormals (smallest, largest, one that is no fp16 number), a value exactly
    between two halves (ties to even, both ways) and ordinary post-ReLU magnitudes."""
    t = np.random.default_rng(11).random((3, 2, 8), dtype=np.float32) * 4
    t[0, 0, :8] = [0.0, 65504.0, 2.0 ** -24, 1023 * 2.0 ** -24, 2.0 ** -24 * 1.5, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -0.0]
    t[2, 1, 7] = 65519.0                                   # rounds down to 65504: still finite
    t[1, 0, 0] = -65504.0
    return t


def test_rounding_is_torch_half_and_non_finite_results_raise():
    t = _edge_table()
    store = FeatureStore(t, device='cpu', dtype='fp16')
    assert store.table.dtype == torch.float16 and tuple(store.table.shape) == (3, 2, 8)
    assert torch.equal(store.table, torch.from_numpy(t).half())
    assert store.loc_table.dtype == torch.float32
    w = store.rows_f32(0)
    assert w.dtype == torch.float32 and torch.equal(w, torch.from_numpy(t).half().float()[0])
    assert float(w[0, 5]) == 1.0 and float(w[0, 6]) == 1.0 + 2.0 ** -9      # ties to even
    assert float(w[0, 2]) == 2.0 ** -24 and float(w[0, 3]) == 1023 * 2.0 ** -24
    big = t.copy()
    big[2, 0, 3] = 65520.0                                 # the smallest magnitude that rounds to inf
    with pytest.raises(ValueError, match='row 2'):
        FeatureStore(big, device='cpu', dtype='fp16')
    nan = t.copy()
    nan[1, 1, 0] = np.nan
    nan[2, 0, 0] = np.nan
    with pytest.raises(ValueError, match='row 1'):
        FeatureStore(nan, device='cpu', dtype='fp16')
    FeatureStore(big, device='cpu')                        # (fp32 storage takes it as before)


def _write_tsv(path, feats):
    with open(path, 'wt') as f:
        for i, feat in enumerate(feats):
            f.write('\t'.join(['scan%d' % (i % 2), 'v%d' % i, '640', '480', '60', base64.b64encode(feat.tobytes()).decode()]) + '\n')


def test_file_format_round_trips_in_both_storages(tmp_path):
    rng = np.random.default_rng(12)
    feats = [(rng.random((36, 2048), dtype=np.float32) * 6).astype(np.float32) for _ in range(5)]
    feats[4][35, 2040:2048] = _edge_table()[0, 0]
    tsv = str(tmp_path / 'f.tsv')
    _write_tsv(tsv, feats)
    want = FeatureStore.from_tsv(tsv, device='cpu', dtype='fp16')
    assert want.table.dtype == torch.float16 and torch.equal(want.table, torch.from_numpy(np.stack(feats)).half())

    b16, b32 = str(tmp_path / 'h.bin'), str(tmp_path / 's.bin')
    assert tsv_to_bin(tsv, b16, dtype='fp16') == 5
    assert tsv_to_bin(tsv, b32) == 5
    assert os.path.getsize(b16) == 5 * 36 * 2048 * 2 and os.path.getsize(b32) == 5 * 36 * 2048 * 4
    with open(b16 + '.json') as f:
        assert json.load(f)['dtype'] == 'float16'
    with open(b32 + '.json') as f:
        assert 'dtype' not in json.load(f)                 # old files and new fp32 files look the same

    a = FeatureStore.from_bin(b16, device='cpu', chunk_rows=2)                     # None: the file's storage
    assert a.dtype == 'fp16' and a.index == want.index and torch.equal(a.table, want.table)
    b = FeatureStore.from_bin(b32, device='cpu', chunk_rows=2, dtype='fp16')       # converted during the upload
    assert b.dtype == 'fp16' and torch.equal(b.table, want.table)
    c = FeatureStore.from_bin(b16, device='cpu', chunk_rows=2, dtype='fp32')       # widened
    assert c.dtype == 'fp32' and c.table.dtype == torch.float32 and torch.equal(c.table, want.table.float())
    d = FeatureStore.from_bin(b32, device='cpu', chunk_rows=3)                     # no "dtype" key: fp32, as before
    assert d.dtype == 'fp32' and torch.equal(d.table, torch.from_numpy(np.stack(feats)))

    feats[3][0, 0] = 70000.0
    _write_tsv(tsv, feats)
    with pytest.raises(ValueError, match='row 3'):
        tsv_to_bin(tsv, str(tmp_path / 'bad.bin'), dtype='fp16')
    tsv_to_bin(tsv, b32)
    with pytest.raises(ValueError, match='row 3'):
        FeatureStore.from_bin(b32, device='cpu', chunk_rows=2, dtype='fp16')


def test_compat_row_read_back_is_fp32():
    from speaker_follower_amd.compat.env import MeanPooledImageFeatures
    t = _edge_table()
    feats = MeanPooledImageFeatures.__new__(MeanPooledImageFeatures)
    feats.store = FeatureStore(t, ids=['s_a', 's_b', 's_c'], device='cpu', dtype='fp16')
    state = types.SimpleNamespace(scanId='s', location=types.SimpleNamespace(viewpointId='b'))
    got = feats.get_features(state)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, torch.from_numpy(t).half().float()[1].numpy())
