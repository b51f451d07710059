"""CPU: the C-ABI library builds, loads, and exports every symbol include/sf_hip.h declares
(no compute calls -- there is no GPU here)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    text = open(os.path.join(ROOT, 'include', 'sf_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(sf_[a-z0-9_]+)\s*\(', text)))


def test_library_builds_and_loads():
    import __graft_entry__
    __graft_entry__.build()
    from speaker_follower_amd import _lib
    assert os.path.exists(_lib.LIB_PATH)
    assert _lib.lib.sf_abi_version() == 10
    from speaker_follower_amd import build
    assert _lib.lib.sf_build_id().decode() == build.build_id() == build.lib_build_id()
    assert _lib.lib.sf_workspace_bytes() >= 32 << 20
    assert _lib.lib.sf_status_string(0) == b'ok'
    assert _lib.lib.sf_status_string(4) == b'workspace too small'


def test_every_header_symbol_is_exported_and_bound():
    import ctypes
    from speaker_follower_amd import _lib
    syms = header_symbols()
    assert len(syms) >= 30
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(raw, s), 'libsf_hip.so does not export %s' % s
    assert set(syms) == set(_lib.EXPORTS), set(syms) ^ set(_lib.EXPORTS)
    # every declaration the reader found is bound with the header's parameter count, and the reader found them all
    assert sorted(_lib.HEADER.functions) == syms and _lib.EXPORTS == tuple(_lib.HEADER.functions)
    for name, decl in _lib.HEADER.functions.items():
        assert len(getattr(_lib.lib, name).argtypes) == len(decl.params), name


def test_missing_header_fails_the_import(monkeypatch, tmp_path):
    import pytest
    from speaker_follower_amd import _lib, build
    assert _lib._headers is build._headers                 # the path the build hashes, not a second expression
    monkeypatch.setattr(_lib, '_headers', lambda: [str(tmp_path / 'sf_hip.h')])
    with pytest.raises(ImportError, match='sf_hip.h is missing'):
        _lib._read_header()


def test_three_signatures_written_by_hand():
    """The reader against something a person wrote: the prototypes of sf_hip.h, re-read by eye."""
    import ctypes as C
    from speaker_follower_amd import _lib
    L, p, i, u32, sz, d = _lib.lib, C.c_void_p, C.c_int, C.c_uint32, C.c_size_t, C.c_double
    P = C.POINTER
    # int sf_linear_fwd(const float* x, int ldx, const float* w, const float* b, int M, int N, int K, int act, float* y,
    #                   int ldy, void* ws, size_t ws_bytes, sf_stream stream)
    assert L.sf_linear_fwd.argtypes == [p, i, p, p, i, i, i, i, p, i, p, sz, p] and L.sf_linear_fwd.restype is i
    assert len(L.sf_linear_fwd.argtypes) == 13
    # int sf_adam_step_dev(float* p, const float* g, float* m, float* v, size_t n, double lr, double beta1, double beta2,
    #                      double eps, double weight_decay, int32_t* step_dev, float* coef,
    #                      const uint32_t* skip_if_nonzero, sf_stream stream)
    assert L.sf_adam_step_dev.argtypes == [p, p, p, p, sz, d, d, d, d, d, p, p, p, p] and L.sf_adam_step_dev.restype is i
    # int sf_encoder_bilstm_fwd(const sf_encoder_w* fwd, const sf_encoder_w* rev, const float* w_e2d, const float* b_e2d,
    #                           const float* w_e2d_t, int B, int Lpad, int T, int E, int H, const int64_t* seq,
    #                           const int32_t* lengths, float* ctx, float* decoder_init, float* c_t,
    #                           const sf_encoder_tape* tape_f, const sf_encoder_tape* tape_r, const sf_dropout* drop,
    #                           uint32_t drop_stream, int32_t* path, void* ws, size_t ws_bytes, sf_stream stream)
    W, T = P(_lib.EncoderW), P(_lib.EncoderTape)
    assert L.sf_encoder_bilstm_fwd.argtypes == [W, W, p, p, p, i, i, i, i, i, p, p, p, p, p, T, T, P(_lib.Dropout), u32,
                                                p, p, sz, p]
    assert L.sf_encoder_bilstm_fwd.restype is i
    assert L.sf_build_id.restype is C.c_char_p and L.sf_workspace_bytes.restype is sz
    assert L.sf_debug_persist_timeout.restype is None and L.sf_profile_end.restype is C.c_long


def test_struct_layouts_match_the_compiler(tmp_path):
    """A second oracle for the derived classes: a C++ program that includes sf_hip.h prints sizeof and every offsetof of
    every struct; each number equals ctypes' for the class built from the reader's fields.  Host only, links nothing."""
    import ctypes as C
    import subprocess
    from speaker_follower_amd import _lib
    structs = _lib.HEADER.structs
    assert len(structs) >= 39 and [c for c, _ in structs] == list(_lib.STRUCTS)
    lines = ['#include <cstdio>', '#include <cstddef>', '#include "sf_hip.h"', 'int main() {']
    for c, fields in structs:
        lines.append('    std::printf("%s %%zu\\n", sizeof(%s));' % (c, c))
        lines += ['    std::printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (c, n, c, n, c, n)
                  for n, _, _ in fields]
    src, exe = tmp_path / 'layout.cpp', tmp_path / 'layout'
    src.write_text('\n'.join(lines + ['    return 0;', '}', '']))
    subprocess.run(['g++', '-std=c++17', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split('\n')
    got = {ln.split()[0]: tuple(int(v) for v in ln.split()[1:]) for ln in out if ln}
    want = {}
    for c, fields in structs:
        cls = _lib.STRUCTS[c]
        assert [n for n, _ in cls._fields_] == [n for n, _, _ in fields], c
        want[c] = (C.sizeof(cls),)
        for n, _, _ in fields:
            want['%s.%s' % (c, n)] = (getattr(cls, n).offset, getattr(cls, n).size)
    assert len(got) == len(want) == len(structs) + sum(len(f) for _, f in structs)
    assert got == want, {k: (got.get(k), want[k]) for k in want if got.get(k) != want[k]}


def test_argument_validation_without_gpu():
    """Entry points reject null pointers / bad sizes before touching the device."""
    from speaker_follower_amd import _lib
    assert _lib.lib.sf_linear_fwd(None, 4, None, None, 1, 1, 4, 0, None, 1, None, 0, None) == 1
    assert _lib.lib.sf_reduce_terms(None, None, 0, 0, None, None) == 1


def test_product_fails_loudly_on_cpu_tensors():
    import pytest
    import torch
    from speaker_follower_amd import model
    m = model.SoftDotAttention(16)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m(torch.zeros(2, 16), torch.zeros(2, 3, 16))
    dec = model.AttnDecoderLSTM(24, 16, 0.5, feature_size=24)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dec(torch.zeros(2, 24), torch.zeros(2, 3, 24), torch.zeros(2, 5, 24), torch.zeros(2, 16),
            torch.zeros(2, 16), torch.zeros(2, 4, 16))
