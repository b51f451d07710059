"""ctypes binding of libsf_hip.so (C ABI in include/sf_hip.h).

There is deliberately NO fallback: if the library is missing or an entry point is
absent, importing this module raises.  A non-zero status from any call raises
SfError.  PyTorch only supplies device memory (`tensor.data_ptr()`) and the
current HIP stream.
"""
import ctypes as C
import os
from itertools import takewhile

# PyTorch-ROCm ships its own HIP runtime (torch/lib/libamdhip64.so, same SONAME as the system
# one).  It must be the first HIP runtime loaded into the process, otherwise libsf_hip.so pulls in
# /opt/rocm's copy and torch -- which provides device memory and streams -- runs on a runtime it was
# not built against.  Importing torch first makes both share torch's runtime.
import torch  # noqa: F401  (load order matters)

from . import _cdecl
from .build import _headers, build_id, CSRC

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, 'libsf_hip.so')


class SfError(RuntimeError):
    pass


def _read_header():
    """include/sf_hip.h is the single source of this binding: every class, argtypes list and constant below is derived
    from its declarations (_cdecl).  The path is the one the build hashes into the library's id."""
    try:
        path = _headers()[-1]
        with open(path) as f:
            return _cdecl.parse(f.read())
    except OSError as e:
        raise ImportError('include/sf_hip.h is missing (%s). The ctypes binding of libsf_hip.so is derived from it; '
                          'there is no hand-written copy to fall back on.' % e)


HEADER = _read_header()

_SCALARS = {'int': C.c_int, 'int32_t': C.c_int32, 'uint32_t': C.c_uint32, 'int64_t': C.c_int64,
            'long long': C.c_longlong, 'uint64_t': C.c_uint64, 'size_t': C.c_size_t, 'long': C.c_long,
            'float': C.c_float, 'double': C.c_double}
# the Python class of struct sf_some_name is SomeName, except for
_NAMES = {'sf_nav_table': 'NavTableS', 'sf_nav_io': 'NavIO', 'sf_nav_routes_io': 'NavRoutesIO',
          'sf_nav_follower_io': 'NavFollowerIO',
          'sf_decoder_gtape': 'DecoderGTape', 'sf_spk_decoder_gtape': 'SpkDecoderGTape'}
# "Gradient structs mirror the weight structs member for member": callers hand a gradient parameter or member the weight
# class filled with gradient pointers.  Held to the header below: same size, and field by field the same offset and size.
_GRAD_AS_WEIGHT = {'sf_lstm_g': 'sf_lstm_w', 'sf_visual_g': 'sf_visual_w', 'sf_softdot_g': 'sf_softdot_w',
                   'sf_scoring_g': 'sf_scoring_w', 'sf_decoder_g': 'sf_decoder_w'}
STRUCTS = {}                         # C name -> class, in header order


def _ctype(ctype, depth, ret=False):
    ctype, extra = HEADER.typedefs.get(ctype, (ctype, 0))          # sf_stream is void*
    ctype, depth = _GRAD_AS_WEIGHT.get(ctype, ctype), depth + extra
    if depth == 0:
        return None if ctype == 'void' else STRUCTS.get(ctype) or _SCALARS[ctype]
    if depth == 1 and ctype in STRUCTS:                             # a struct defined further down stays void*
        return C.POINTER(STRUCTS[ctype])
    return C.c_char_p if ret and (ctype, depth) == ('char', 1) else C.c_void_p


def _layout(cls):
    return [C.sizeof(cls)] + [(getattr(cls, n).offset, getattr(cls, n).size) for n, _ in cls._fields_]


for _c, _fields in HEADER.structs:
    _py = _NAMES.get(_c) or ''.join(p.capitalize() for p in _c[3:].split('_'))
    STRUCTS[_c] = globals()[_py] = type(_py, (C.Structure,), {
        '__doc__': _c, '_fields_': [(n, _ctype(t, d)) for n, t, d in _fields]})
    if _c in _GRAD_AS_WEIGHT and _layout(STRUCTS[_c]) != _layout(STRUCTS[_GRAD_AS_WEIGHT[_c]]):
        raise ImportError('sf_hip.h: %s no longer mirrors %s member for member' % (_c, _GRAD_AS_WEIGHT[_c]))

# the leading sizes and the trailing tables of sf_state_search, by name (search.py fills them from dicts)
_f = StateSearch._fields_                                          # noqa: F821  (defined by the loop above)
StateSearch.SIZES = tuple(n for n, _ in takewhile(lambda f: f[1] is C.c_int32, _f))                   # noqa: F821
StateSearch.POINTERS = tuple(n for n, _ in takewhile(lambda f: f[1] is C.c_void_p, reversed(_f)))[::-1]   # noqa: F821

globals().update(HEADER.constants)   # SF_OK ... SF_ERR_WORKSPACE, SF_ENC_*, SF_SPK_EMB_DROPOUT, SF_EVAL_MAX_GOLD, ...
ABI_VERSION = HEADER.constants['SF_ABI_VERSION']
SEARCH_OVF_NODES, SEARCH_OVF_SLOTS, SEARCH_OVF_VISITS, SEARCH_OVF_POOL, SEARCH_OVF_KEY = (
    HEADER.constants['SF_SEARCH_OVF_' + n] for n in ('NODES', 'SLOTS', 'VISITS', 'POOL', 'KEY'))
EXPORTS = tuple(HEADER.functions)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            'libsf_hip.so is missing (%s). Build it with `python -m speaker_follower_amd.build`; '
            'there is no CPU fallback for the speaker/follower hot path.' % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, decl in HEADER.functions.items():
        fn = getattr(lib, name)            # AttributeError if the symbol is not exported
        fn.restype = _ctype(*decl.ret, ret=True)
        fn.argtypes = [_ctype(t, d) for _, t, d in decl.params]
    if lib.sf_abi_version() != ABI_VERSION:
        raise ImportError('libsf_hip.so ABI version mismatch')
    # a library built from other sources than the ones on disk (stale .so after a checkout) is refused
    if os.path.isdir(CSRC) and os.environ.get('SF_SKIP_BUILD_ID_CHECK') != '1':
        have, want = lib.sf_build_id().decode(), build_id()
        if have != want:
            raise ImportError('libsf_hip.so is stale: built from sources %s, the tree holds %s; run '
                              '`python -m speaker_follower_amd.build`' % (have, want))
    return lib


lib = _load()

def check(status, what=''):
    if status != 0:
        detail = lib.sf_status_string(status).decode()
        if status == 3:
            detail += ': ' + lib.sf_last_error_string().decode()
        raise SfError('%s failed: %s (status %d)' % (what or 'libsf_hip call', detail, status))


def call(name, *args):
    check(getattr(lib, name)(*args), name)


class kernel_profile:
    """`with kernel_profile() as prof: ...` times every kernel this thread launches through the
    library (sf_profile_begin / sf_profile_end); afterwards prof.rows maps the kernel name to
    dict(calls, total_us, avg_us, min_us, max_us).  Eager issue only (not under graph capture)."""

    def __init__(self, library=None):
        self.library = library if library is not None else lib

    def __enter__(self):
        check(self.library.sf_profile_begin(), 'sf_profile_begin')
        self.rows = {}
        return self

    def __exit__(self, *exc):
        buf = C.create_string_buffer(1 << 16)
        n = self.library.sf_profile_end(buf, len(buf))
        if n < 0:
            raise SfError('sf_profile_end failed')
        for line in buf.value.decode().splitlines():
            name, calls, total, mn, mx = line.split('\t')
            name = name.strip('()')
            self.rows[name] = dict(calls=int(calls), total_us=float(total), avg_us=float(total) / int(calls),
                                   min_us=float(mn), max_us=float(mx))
        return False
