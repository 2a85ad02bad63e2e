"""Reader of the C boundary's headers (``include/pyg_amd.h``, ``include/pyg_amd_lab.h``).

The headers are plain, regular C99: ``#define PYGAMD_X <integer>`` constants, ``typedef enum`` with
explicit values, ``typedef struct`` argument blocks and one ``PYGAMD_API <ret> name(<params>);`` per
entry point.  :func:`parse` reads exactly that and raises :class:`PygAmdError` on anything else —
it never guesses and never skips — and :func:`ctype` is the one map from a C type to ctypes.
``_lib.py`` derives its whole binding from the two; nothing restates the header by hand.
"""
import re
from collections import namedtuple
from ctypes import (POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t,
                    c_uint64, c_void_p)


class PygAmdError(RuntimeError):
    pass


# functions: name -> (return C type, [parameter C types]); structs: typedef name -> [(field, C type,
# array length or None)]; constants: name -> int.  C types in one spelling: 'const float*',
# 'int64_t', 'float* const*', ...
Header = namedtuple('Header', 'functions structs constants')

SCALARS = {'int': c_int, 'int32_t': c_int32, 'int64_t': c_int64, 'uint64_t': c_uint64,
           'size_t': c_size_t, 'float': c_float, 'double': c_double}
# what a pointer other than `const char*` (a return type) or a struct pointer may point to
POINTEES = {'void', 'float', 'double', 'int32_t', 'uint32_t', 'int64_t', 'uint64_t', 'size_t'}

_TYPE = re.compile(r'(const )?(\w+)(\*(?: const\*)?)?$')
_DEFINE = re.compile(r'#\s*define\s+(PYGAMD_\w+)\b(.*)')
_ENUM = re.compile(r'typedef\s+enum\s*\{([^{}]*)\}\s*\w+\s*;')
_STRUCT = re.compile(r'typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;')
_FUNCTION = re.compile(r'PYGAMD_API\s+([\w\s*]+?)\b(\w+)\s*\(([^()]*)\)\s*;')
_DECLARATOR = re.compile(r'(.+?)\b(\w+)\s*(?:\[\s*(\d+)\s*\])?$', re.S)


def _integer(value, where):
    try:
        return int(value, 0)
    except ValueError:
        raise PygAmdError(f'{where}: expected an integer value, got "{value}"') from None


def parse(text, included=None):
    """Read header ``text``; the structs of ``included`` (the :class:`Header` of a header that
    ``text`` includes) may be pointed to as well."""
    functions, structs, constants = {}, {}, {}
    known = set(included.structs) if included else set()

    def c_type(spelling, where, ret=False):
        t = re.sub(r'\s*\*\s*', '* ', ' '.join(spelling.split())).strip()
        m = _TYPE.match(t)
        const, base, ptr = m.groups() if m else (None, None, None)
        if not (base in SCALARS and not const if not ptr else
                base in POINTEES or (base in known and ptr == '*') or (ret and t == 'const char*')):
            raise PygAmdError(f'{where}: unknown type "{t}"')
        return t

    def declarator(decl, where):
        m = _DECLARATOR.match(decl.strip())
        if not m:
            raise PygAmdError(f'{where}: cannot read "{" ".join(decl.split())}"')
        return m.group(2), c_type(m.group(1), f'{where}, {m.group(2)}'), m.group(3)

    def enum(m):
        for item in filter(None, map(str.strip, m.group(1).split(','))):
            name, eq, value = map(str.strip, item.partition('='))
            if not eq:
                raise PygAmdError(f'enumerator {name} has no explicit value')
            constants[name] = _integer(value, f'enumerator {name}')
        return ''

    def struct(m):
        name = m.group(2)
        fields = [declarator(d, f'struct {name}') for d in m.group(1).split(';') if d.strip()]
        structs[name] = [(f, t, int(n) if n else None) for f, t, n in fields]
        known.add(name)
        return ''

    def function(m):
        ret, name, params = m.groups()
        params = [] if params.strip() == 'void' else params.split(',')
        types = []
        for p in params:
            _, t, n = declarator(p, name)
            if n:
                raise PygAmdError(f'{name}: array parameter "{" ".join(p.split())}"')
            types.append(t)
        functions[name] = (c_type(ret, f'{name}, return type', ret=True), types)
        return ''

    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    code = []
    for line in text.splitlines():
        if not line.lstrip().startswith('#'):
            code.append(line)
            continue
        m = _DEFINE.match(line.strip())
        if m and m.group(1) != 'PYGAMD_API':   # (the export attribute itself)
            constants[m.group(1)] = _integer(m.group(2).strip(), f'#define {m.group(1)}')
    rest = '\n'.join(code).replace('extern "C" {', '', 1)
    for pattern, reader in ((_ENUM, enum), (_STRUCT, struct), (_FUNCTION, function)):
        rest = pattern.sub(reader, rest)
    rest = ' '.join(rest.split())
    if rest not in ('', '}'):   # '}' closes the extern "C" block
        raise PygAmdError(f'cannot read the declaration "{rest[:160]}"')
    return Header(functions, structs, constants)


def ctype(spelling, mirrors):
    """The ctypes type of a C type as :func:`parse` spells it.  ``mirrors``: typedef name ->
    ``ctypes.Structure`` of the header's structs.  Every pointer that is neither ``const char*`` nor
    a struct pointer is ``c_void_p``, which takes what callers pass: ``tensor.data_ptr()``,
    ``None``, ``ctypes.byref(...)`` and ctypes arrays."""
    _, base, ptr = _TYPE.match(spelling).groups()
    if not ptr:
        return SCALARS[base]
    if base == 'char':
        return c_char_p
    if base in POINTEES:
        return c_void_p
    if base not in mirrors:
        raise PygAmdError(f'no ctypes mirror of struct {base}')
    return POINTER(mirrors[base])


def fields(struct):
    """``_fields_`` of the ctypes mirror of one of ``Header.structs``."""
    return [(f, ctype(t, {}) * n if n else ctype(t, {})) for f, t, n in struct]


def signatures(header, mirrors):
    """name -> (restype, argtypes) of every function of ``header``."""
    return {name: (ctype(ret, mirrors), [ctype(t, mirrors) for t in params])
            for name, (ret, params) in header.functions.items()}
