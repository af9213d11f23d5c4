"""The ctypes view of include/psnerf_hip.h, read from the header itself: parse(path) -> (constants, structs, functions).

The header is ours and is written in a narrow, regular style; the grammar below covers exactly that style and nothing else.
Whatever it does not cover -- an unknown type, a bit-field, a function-pointer parameter, a preprocessor line in the middle of a
declaration -- raises HeaderError with the header line: the parser never guesses and never skips.  Pure Python + ctypes (no
torch, no library load), so it can be used and tested without the shared library.
"""
import ctypes
import re

SCALARS = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'long long': ctypes.c_longlong,
           'float': ctypes.c_float, 'double': ctypes.c_double, 'uint8_t': ctypes.c_uint8, 'uint16_t': ctypes.c_uint16,
           'uint32_t': ctypes.c_uint32, 'unsigned char': ctypes.c_ubyte, 'unsigned long long': ctypes.c_ulonglong}
POINTEES = ('void', 'char')     # legal behind a '*' in addition to the scalars and the Psn structs

_SPACE = re.compile(r'\s*')
_DIRECTIVE = re.compile(r'#.*')
_ENUM = re.compile(r'enum\s*\{([^{}]*)\}\s*;')
_STRUCT = re.compile(r'typedef\s+struct\s*\{([^{}]*)\}\s*(Psn\w+)\s*;')
_FUNC = re.compile(r'([\w\s*]+?)\b(psn_\w+)\s*\(([^(){};]*)\)\s*;')
_DECLARATOR = r'\w+(?:\s*\[[^\]]+\])?'
_FIELDS = re.compile(r'([\w\s]+?)\s+(%s(?:\s*,\s*%s)*)' % (_DECLARATOR, _DECLARATOR))
_INT = re.compile(r'(0[xX][0-9a-fA-F]+|\d+)(?:[uU]?[lL]{0,2})')


class HeaderError(ValueError):
    pass


def parse(path):
    with open(path) as f:
        text = f.read()
    blank = lambda m: '\n' * m.group(0).count('\n')     # (line numbers survive every deletion)
    text = re.sub(r'/\*.*?\*/', blank, text, flags=re.S)
    text = re.sub(r'^#ifdef __cplusplus\n(extern "C" \{|\})\n#endif\n', blank, text, flags=re.M)
    text = re.sub(r'\A\s*#ifndef (\w+)\n#define \1\n', blank, text)     # the include guard: first and last directive
    text = re.sub(r'^#endif\s*\Z', blank, text, flags=re.M)
    constants, structs, functions = {}, {}, {}

    def fail(pos, what):
        raise HeaderError('%s:%d: %s' % (path, text.count('\n', 0, pos) + 1, what))

    def integer(expr, pos):
        """An integer constant expression over literals, known constants, + - * and parentheses."""
        out = []
        for tok in re.findall(r'\w+|\S', expr):
            if tok in constants:
                out.append(str(constants[tok]))
            elif _INT.fullmatch(tok):
                out.append(str(int(_INT.fullmatch(tok).group(1), 0)))
            elif tok in '+-*()':
                out.append(tok)
            else:
                fail(pos, 'not an integer constant expression: %r' % expr.strip())
        try:
            return int(eval(' '.join(out), {'__builtins__': {}}))
        except Exception:
            fail(pos, 'not an integer constant expression: %r' % expr.strip())

    def ctype(name, pos):
        name = ' '.join(name.split())
        if name not in SCALARS and name not in structs:
            fail(pos, 'unknown type %r' % name)
        return SCALARS.get(name) or structs[name]

    def pointer(decl, pos):
        """'const T* [const*] name' -> c_void_p, after a look at T."""
        base = ' '.join(w for w in decl.split('*')[0].split() if w != 'const')
        if base not in POINTEES:
            ctype(base, pos)
        if not re.fullmatch(r'[\w\s]+\*(\s*const\s*\*)?\s*\w+', decl):
            fail(pos, 'pointer declaration outside the grammar: %r' % decl)
        return ctypes.c_void_p

    def fields(body, pos):
        out = []
        for decl in (d.strip() for d in body.split(';')):
            if '*' in decl:
                out.append((decl.rsplit('*', 1)[1].strip(), pointer(decl, pos)))
            elif decl:
                m = _FIELDS.fullmatch(decl)
                if not m:
                    fail(pos, 'field declaration outside the grammar: %r' % decl)
                for d in m.group(2).split(','):
                    name, _, dim = d.strip().partition('[')
                    t = ctype(m.group(1), pos)
                    out.append((name.strip(), t * integer(dim.rstrip(' ]'), pos) if dim else t))
        return out

    def params(plist, pos):
        out = []
        for p in ([] if plist.strip() == 'void' else plist.split(',')):
            if '*' in p:
                out.append(pointer(p.strip(), pos))
                continue
            m = re.fullmatch(r'\s*([\w\s]+?)\s+\w+\s*', p)
            out.append(ctype(m.group(1), pos) if m else fail(pos, 'parameter outside the grammar: %r' % p.strip()))
        return out

    def directive(m, pos):
        d = re.fullmatch(r'#define\s+(PSN_\w+)\s+(.+)', m.group(0))
        if d:
            constants[d.group(1)] = integer(d.group(2), pos)
        elif not re.fullmatch(r'#include\s*<[\w./]+>\s*', m.group(0)):
            fail(pos, 'preprocessor line outside the grammar: %r' % m.group(0))

    def enum(m, pos):
        value = -1
        for item in m.group(1).split(','):
            name, eq, expr = item.partition('=')
            if not re.fullmatch(r'\s*PSN_\w+\s*', name):
                fail(pos, 'enumerator outside the grammar: %r' % item.strip())
            value = constants[name.strip()] = integer(expr, pos) if eq else value + 1

    def struct(m, pos):
        structs[m.group(2)] = type(m.group(2), (ctypes.Structure,), {'_fields_': fields(m.group(1), pos)})

    def function(m, pos):
        ret = ' '.join(m.group(1).split())
        functions[m.group(2)] = (ctypes.c_char_p if ret == 'const char*' else ctype(ret, pos), params(m.group(3), pos))

    pos = _SPACE.match(text).end()
    while pos < len(text):      # one declaration after the other; whatever none of the four forms matches is an error
        for form, take in ((_DIRECTIVE, directive), (_ENUM, enum), (_STRUCT, struct), (_FUNC, function)):
            m = form.match(text, pos)
            if m:
                take(m, pos)
                break
        else:
            fail(pos, 'declaration outside the grammar: %r' % text[pos:pos + 60].split('\n')[0])
        pos = _SPACE.match(text, m.end()).end()
    for m in re.finditer(r'\b(psn_\w+)\s*\(', text):
        if m.group(1) not in functions:
            fail(m.start(), '%s( did not become a function' % m.group(1))
    return constants, structs, functions
