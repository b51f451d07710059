"""Reader of the declarations in include/sf_hip.h: the one place the C ABI of libsf_hip.so is written down.

`parse(text)` returns a Header of
    structs    [(name, [(field, C type, pointer depth)])]          in header order
    functions  {name: Function(ret=(C type, depth), params=[(name, C type, depth)], line)}
    constants  {name: int}       every `#define NAME <integer>` and every enum member
    typedefs   {name: (C type, depth)}                              sf_stream
C types are spelled without `const` / `struct` ('float', 'long long', 'sf_pano').  This is no C parser: it knows the
forms that header uses and refuses everything else -- arrays, bit-fields, unions, function pointers, variadics, unknown
type names, other preprocessor lines -- with a ValueError naming the line.  A declaration it skipped would be a binding
missing at call time.  Pure Python: neither torch nor the library is imported.
"""
import re
from collections import namedtuple

Header = namedtuple('Header', 'structs functions constants typedefs')
Function = namedtuple('Function', 'ret params line')

SCALARS = ('void', 'char', 'int', 'long', 'long long', 'unsigned long long', 'float', 'double', 'size_t', 'int32_t',
           'uint32_t', 'int64_t', 'uint64_t', 'uint8_t')
_TOKEN = re.compile(r'[A-Za-z_]\w*|-?\d\w*|\.\.\.|\S')


def _fail(line, msg):
    raise ValueError('line %d: %s' % (line, msg))


def _integer(tok, line):
    try:
        return int(tok, 0)
    except ValueError:
        _fail(line, 'expected an integer, found %r' % tok)


class _Reader:
    def __init__(self, text):
        self.structs, self.functions, self.constants, self.typedefs = {}, {}, {}, {}
        self.declared, self.forward = {}, {}
        # a comment leaves its newlines behind, so that tokens keep their line numbers
        text = re.sub(r'/\*.*?\*/|//[^\n]*', lambda m: '\n' * m.group().count('\n') or ' ', text, flags=re.S)
        lines = text.split('\n')
        self.preprocessor(lines)
        self.toks, self.lines, self.i = [], [], 0              # token i stands on line lines[i]; '' ends the file
        for n, s in enumerate(lines, 1):
            found = _TOKEN.findall(s)
            self.toks += found
            self.lines += [n] * len(found)
        self.toks += [''] * 3                                  # (peek looks at most two tokens ahead)
        self.lines += [len(lines)] * 3
        while self.peek():
            {'typedef': self.typedef, 'enum': self.enum}.get(self.peek(), self.function)()
        for name, line in self.forward.items():
            if name not in self.structs:
                _fail(line, 'struct %s is never defined' % name)

    def preprocessor(self, lines):
        """#define NAME <integer> -> constants; the include guard, #include and the extern "C" guards are dropped."""
        guard, open_ifs = None, []
        for n, raw in enumerate(lines, 1):
            s = raw.strip()
            if not s.startswith('#'):
                if 'cplusplus' in open_ifs:
                    if s not in ('', 'extern "C" {', '}'):
                        _fail(n, 'only the extern "C" guards may stand under #ifdef __cplusplus')
                    lines[n - 1] = ''
                continue
            lines[n - 1] = ''
            d = s[1:].split()
            if d[:1] == ['include'] or (d == ['define', guard] and guard):
                pass
            elif d == ['ifdef', '__cplusplus']:
                open_ifs.append('cplusplus')
            elif d[:1] == ['ifndef'] and len(d) == 2 and guard is None:
                guard = d[1]
                open_ifs.append('guard')
            elif d == ['endif'] and open_ifs:
                open_ifs.pop()
            elif d[:1] == ['define'] and len(d) == 3 and d[1].isidentifier():
                self.declare(d[1], n)
                self.constants[d[1]] = _integer(d[2], n)
            else:
                _fail(n, 'unsupported preprocessor line %r' % s)
        if open_ifs:
            _fail(len(lines), 'unterminated #if')

    # ---- tokens
    def peek(self, ahead=0):
        return self.toks[self.i + ahead]

    def line(self):
        return self.lines[self.i]

    def take(self, want=None):
        tok, line = self.toks[self.i], self.lines[self.i]
        if (want is not None and tok != want) or (want is None and not tok.isidentifier()):
            _fail(line, 'expected %s, found %r' % (repr(want) if want else 'a name', tok or 'end of file'))
        self.i += 1
        return tok

    def declare(self, name, line):
        if name in self.declared:
            _fail(line, '%s is declared twice (first at line %d)' % (name, self.declared[name]))
        self.declared[name] = line

    # ---- declarations
    def type(self):
        while self.peek() == 'const':
            self.take()
        line = self.line()
        if self.peek() == '...':
            _fail(line, 'variadic parameter lists are not supported')
        tok = self.take()
        if tok == 'union':
            _fail(line, 'unions are not supported')
        if tok == 'struct':                                  # `struct X`: the only way to name a struct defined later
            tok = self.take()
            if tok not in self.structs:
                self.forward.setdefault(tok, line)
        else:
            while tok.endswith(('unsigned', 'long')) and self.peek() == 'long':
                tok += ' ' + self.take()                      # long long, unsigned long long
            if tok not in SCALARS and tok not in self.typedefs and tok not in self.structs:
                _fail(line, 'unknown type name %r' % tok)
        while self.peek() == 'const':
            self.take()
        return tok

    def declarator(self, ctype, named=True):
        depth, line = 0, self.line()
        while self.peek() in ('*', 'const'):
            depth += self.take(self.peek()) == '*'
        if self.peek() == '(':
            _fail(line, 'function pointers are not supported')
        name = self.take() if named else None
        if self.peek() == '[':
            _fail(line, 'array %s: arrays are not supported' % name)
        if self.peek() == ':':
            _fail(line, 'bit-field %s: bit-fields are not supported' % name)
        if depth == 0 and named and (ctype == 'void' or (ctype not in self.structs and ctype in self.forward)):
            _fail(line, '%s has incomplete type %s' % (name, ctype))
        return name, ctype, depth

    def members(self, close, sep, start):
        """Declarations up to `close`: fields (`;` behind each, several declarators per type) or parameters (`,`)."""
        out, seen = [], set()

        def member(ctype):
            line = self.line()
            out.append(self.declarator(ctype))
            if out[-1][0] in seen:
                _fail(line, 'member %s is declared twice' % out[-1][0])
            seen.add(out[-1][0])

        while self.peek() != close:
            if not self.peek():
                _fail(start, 'unterminated %s' % ('struct' if close == '}' else 'parameter list'))
            ctype = self.type()
            member(ctype)
            while sep == ';' and self.peek() == ',':
                self.take(',')
                member(ctype)
            if sep == ';' or self.peek() != close:
                self.take(sep)
        self.take(close)
        return out

    def typedef(self):
        line = self.line()
        self.take('typedef')
        if self.peek() == 'struct' and self.peek(2) == '{':
            self.take('struct')
            name = self.take()
            self.declare(name, line)
            self.take('{')
            fields = self.members('}', ';', line)
            self.take(name)                                  # typedef struct X { ... } X;
            self.structs[name] = fields
        else:
            name, ctype, depth = self.declarator(self.type())
            self.declare(name, line)
            self.typedefs[name] = (ctype, depth)
        self.take(';')

    def enum(self):
        self.take('enum')                                    # enum { NAME = <integer>, ... };
        self.take('{')
        while self.peek() != '}':
            line, name = self.line(), self.take()
            self.declare(name, line)
            self.take('=')
            self.constants[name] = _integer(self.peek(), self.line())
            self.i += 1
            if self.peek() != '}':
                self.take(',')
        self.take('}')
        self.take(';')

    def function(self):
        _, ctype, depth = self.declarator(self.type(), named=False)
        line, name = self.line(), self.take()
        self.declare(name, line)
        self.take('(')
        if self.peek() == 'void' and self.peek(1) == ')':
            self.take('void')
        self.functions[name] = Function((ctype, depth), self.members(')', ',', line), line)
        self.take(';')


def parse(text):
    r = _Reader(text)
    return Header(list(r.structs.items()), r.functions, r.constants, r.typedefs)
