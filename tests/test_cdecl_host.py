"""CPU: the declaration reader behind the ctypes binding (speaker_follower_amd/_cdecl.py) on short synthetic headers --
every form include/sf_hip.h uses is read, every form it does not use is refused with the line named.  Neither torch nor
the library is needed."""
import os
import re

import pytest

from speaker_follower_amd import _cdecl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def refused(text, line, word):
    with pytest.raises(ValueError, match=r'line %d: .*%s' % (line, word)):
        _cdecl.parse(text)


@pytest.mark.parametrize('text, line, word', [
    ('typedef struct sf_a {\n    int n;\n    float v[4];\n} sf_a;\n', 3, 'array'),
    ('typedef struct sf_a {\n    int n : 3;\n} sf_a;\n', 2, 'bit-field'),
    ('\n\ntypedef union sf_u { int i; float f; } sf_u;\n', 3, 'union'),
    ('typedef struct sf_a {\n    union { int i; float f; } u;\n} sf_a;\n', 2, 'union'),
    ('int sf_f(int n,\n         void (*cb)(int));\n', 2, 'function pointer'),
    ('typedef struct sf_a {\n    int (*cb)(void);\n} sf_a;\n', 2, 'function pointer'),
    ('int sf_f(const char* fmt,\n         ...);\n', 2, 'variadic'),
    ('int sf_f(int n);\nint sf_g(uint16_t n);\n', 2, "unknown type name 'uint16_t'"),
    ('typedef struct sf_a {\n    sf_b inner;\n} sf_a;\n', 2, "unknown type name 'sf_b'"),
    ('int sf_f(void);\ntypedef struct sf_a {\n    int n;\n', 2, 'unterminated struct'),
    ('int sf_f(void);\n\nint sf_f(int n);\n', 3, 'sf_f is declared twice'),
    ('typedef struct sf_a { int n; } sf_a;\ntypedef struct sf_a { int n; } sf_a;\n', 2, 'sf_a is declared twice'),
    ('#define SF_X 1\nenum { SF_Y = 2,\n       SF_X = 3 };\n', 3, 'SF_X is declared twice'),
    ('typedef struct sf_a {\n    int n;\n    float n;\n} sf_a;\n', 3, 'member n is declared twice'),
])
def test_unknown_forms_are_refused_with_their_line(text, line, word):
    refused(text, line, word)


@pytest.mark.parametrize('text, line', [
    ('#if SF_WIDE\nint sf_f(void);\n#endif\n', 1),                      # conditional declarations
    ('#define SF_MAX(a, b) ((a) > (b) ? (a) : (b))\n', 1),             # function-like macro
    ('#define SF_PI 3.14\n', 1),                                        # not an integer
    ('int sf_f(void);\nstatic int sf_g(void);\n', 2),                   # storage class
    ('typedef struct sf_a {\n    int n;\n} sf_b;\n', 3),                 # tag and typedef name differ
    ('typedef struct sf_a {\n    struct sf_later s;\n} sf_a;\n', 2),     # incomplete type by value
    ('int sf_f(const struct sf_never* p);\n', 1),                       # forward reference never resolved
    ('int sf_f(int n)\nint sf_g(void);\n', 2),                          # missing semicolon
    ('enum {\n    SF_A = 0,\n    SF_B };\n', 3),                          # an enumerator without its value
    ('enum sf_status { SF_A = 0 };\n', 1),                             # a named enum (a type nothing here could use)
])
def test_nothing_is_skipped(text, line):
    refused(text, line, '')


HEADER = '''/* a comment with int sf_hidden(void); inside
 * over two lines */
#ifndef SF_T_H_
#define SF_T_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define SF_X 7
enum { SF_A = 0, SF_B = 4,
       SF_D = 0x10 };   // trailing comment
typedef void* sf_stream;
typedef struct sf_inner {
    const float *w_ih, *w_hh;      /* two pointers */
    int32_t V, IMG, LOC;
} sf_inner;
typedef struct sf_outer {
    sf_inner lstm;
    const sf_inner* first;
    const struct sf_later* nav;
    long long steps;
    uint8_t** rows;
} sf_outer;
typedef struct sf_later { double margin; } sf_later;
int sf_three(const sf_outer* o, int B /* rows */,
             const float* x,
             size_t ws_bytes, sf_stream stream);
size_t sf_none(void);
const char* sf_name(int status);
void sf_trace(unsigned long long* buf);
#ifdef __cplusplus
}
#endif
#endif /* SF_T_H_ */
'''


def test_every_form_of_the_header_is_read():
    h = _cdecl.parse(HEADER)
    assert h.constants == {'SF_X': 7, 'SF_A': 0, 'SF_B': 4, 'SF_D': 16}      # no SF_T_H_: the guard
    assert h.typedefs == {'sf_stream': ('void', 1)}
    assert h.structs == [
        ('sf_inner', [('w_ih', 'float', 1), ('w_hh', 'float', 1), ('V', 'int32_t', 0), ('IMG', 'int32_t', 0),
                      ('LOC', 'int32_t', 0)]),
        ('sf_outer', [('lstm', 'sf_inner', 0), ('first', 'sf_inner', 1), ('nav', 'sf_later', 1),
                      ('steps', 'long long', 0), ('rows', 'uint8_t', 2)]),
        ('sf_later', [('margin', 'double', 0)])]
    assert list(h.functions) == ['sf_three', 'sf_none', 'sf_name', 'sf_trace']
    f = h.functions['sf_three']
    assert (f.ret, f.line) == (('int', 0), 25)
    assert f.params == [('o', 'sf_outer', 1), ('B', 'int', 0), ('x', 'float', 1), ('ws_bytes', 'size_t', 0),
                        ('stream', 'sf_stream', 0)]
    assert h.functions['sf_none'] == (('size_t', 0), [], 28)
    assert h.functions['sf_name'].ret == ('char', 1)
    assert h.functions['sf_trace'] == (('void', 0), [('buf', 'unsigned long long', 1)], 30)


def test_the_package_header_is_read_whole():
    with open(os.path.join(ROOT, 'include', 'sf_hip.h')) as f:
        text = f.read()
    h = _cdecl.parse(text)
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)                   # the count of a plain search: nothing dropped
    assert [s for s, _ in h.structs] == re.findall(r'typedef struct (\w+) \{', text) and len(h.structs) >= 39
    assert sorted(h.functions) == sorted(set(re.findall(r'\b(sf_[a-z0-9_]+)\s*\(', text))) and len(h.functions) >= 123   # (125 less the two retired entries)
    assert sorted(n for n in h.constants if n not in ('SF_OK',) and not n.startswith(('SF_ERR_', 'SF_SEARCH_OVF_'))) == \
        sorted(re.findall(r'#define (SF_\w+) \d+', text))
    assert h.typedefs == {'sf_stream': ('void', 1)}
    assert h.constants['SF_ABI_VERSION'] == 10 and h.constants['SF_SEARCH_OVF_KEY'] == 16
    assert 'SF_HIP_H_' not in h.constants
    assert ('nav', 'sf_nav_io', 1) in dict(h.structs)['sf_follower_glue']          # the one forward reference
