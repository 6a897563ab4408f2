"""Reader of include/xmem_hip.h: the header is the one declaration of the C ABI, `_lib` binds what `parse` returns.

Dialect (anything else raises ValueError naming the text; nothing is skipped): /* */ and // comments, preprocessor lines (of which
`#define XMEM_NAME <integer>` is kept), `extern "C" {` and its `}`, `typedef enum {..} name;` / `enum {..};` of `XMEM_NAME = <integer>`,
`typedef struct {..} name;` of scalar, pointer and array fields (several declarators per statement; an array sized by a literal or a
#define), and prototypes `type xmem_name(type name, ..);` or `(void)`.  `const` may stand anywhere.

Type rules: int, float, double, size_t, uint64_t, int32_t, uint8_t -> c_int, c_float, c_double, c_size_t, c_uint64, c_int32, c_uint8.
Struct* -> POINTER(Struct), Struct** -> POINTER(POINTER(Struct)), size_t* -> POINTER(c_size_t), void** -> POINTER(c_void_p), a
`const char*` return -> c_char_p, every other pointer (device memory, streams, workspaces) -> c_void_p.  The field `in` is named `inp`.
"""
import ctypes as C
import re

SCALARS = {'int': C.c_int, 'float': C.c_float, 'double': C.c_double, 'size_t': C.c_size_t, 'uint64_t': C.c_uint64,
           'int32_t': C.c_int32, 'uint8_t': C.c_uint8}
POINTEES = set(SCALARS) | {'void', 'char', 'int8_t', 'uint16_t', 'uint32_t'}     # what a plain c_void_p may point to
FIELD_NAMES = {'in': 'inp'}                                             # Python keywords
_ENUM = r'(?:typedef\s+)?enum\s*\{([^{}]*)\}\s*\w*\s*;'
_STRUCT = r'typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;'
_PROTO = r'([\w\s*]+?)\b(xmem_[a-z0-9_]+)\s*\(([^()]*)\)\s*;'


def _ctype(text, structs, ret=False):
    """ctypes type of a C type written as words and stars (`const xmem_conv_desc* const*`)."""
    words = re.sub(r'\bconst\b', ' ', text).replace('*', ' * ').split()
    base, stars = (words or [''])[0], len(words) - 1
    if words[1:] == ['*'] * stars:
        if base in structs or (base in SCALARS and (stars == 0 or base == 'size_t')):
            t = structs.get(base) or SCALARS[base]
            for _ in range(stars):
                t = C.POINTER(t)
            return t
        if base == 'void' and stars == 2:
            return C.POINTER(C.c_void_p)
        if base in POINTEES and stars == 1:
            return C.c_char_p if ret and base == 'char' else C.c_void_p
    raise ValueError(f'unknown type: {text.strip()!r}')


def _integer(text, constants, what):
    text = text.strip()
    if re.fullmatch(r'-?\d+', text):
        return int(text)
    if text in constants:
        return constants[text]
    raise ValueError(f'{what}: {text!r} is not an integer')


def _fields(body, structs, constants):
    fields = []
    for stmt in filter(None, (s.strip() for s in body.split(';'))):
        first, *more = stmt.split(',')
        m = re.fullmatch(r'(.*?[\s*])(\w+)\s*(\[[^\]]*\])?', first, re.S)
        if not m:
            raise ValueError(f'cannot split declarator: {stmt!r}')
        ctype = _ctype(m.group(1), structs)
        for decl in [m.group(2) + (m.group(3) or '')] + more:
            d = re.fullmatch(r'\s*(\w+)\s*(?:\[([^\]]*)\])?\s*', decl)
            if not d:
                raise ValueError(f'cannot split declarator: {stmt!r}')
            n = d.group(2)
            fields.append((FIELD_NAMES.get(d.group(1), d.group(1)),
                           ctype if n is None else ctype * _integer(n, constants, f'array size of {d.group(1)}')))
    return fields


def parse(text):
    """(constants, structs, functions) of a header: name -> int, name -> ctypes.Structure subclass, name -> (restype, [argtypes])."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    n_functions = len(set(re.findall(r'\b(xmem_[a-z0-9_]+)\s*\(', text)))
    n_structs = len(re.findall(r'\btypedef\s+struct\b', text))
    constants, structs, functions = {}, {}, {}

    def define(m):
        if m.group(1):
            constants[m.group(1)] = _integer(m.group(2), constants, m.group(1))
        return ''
    text = re.sub(r'^[ \t]*#[ \t]*(?:define[ \t]+(XMEM_\w+)[ \t]+(\S[^\n]*)|[^\n]*)$', define, text, flags=re.M)
    text, n_extern = re.subn(r'extern\s+"C"\s*\{', '', text)

    def enum(m):
        value = -1
        for item in filter(None, (s.strip() for s in m.group(1).split(','))):
            name, eq, number = item.partition('=')
            if not re.fullmatch(r'XMEM_\w+', name.strip()):
                raise ValueError(f'cannot split enumerator: {item!r}')
            value = constants[name.strip()] = _integer(number, constants, name.strip()) if eq else value + 1
        return ''
    text = re.sub(_ENUM, enum, text)
    # in the order of the header: a struct or prototype may name only the structs declared above it
    for m in re.finditer(f'{_STRUCT}|{_PROTO}', text):
        if m.group(2):
            structs[m.group(2)] = type(m.group(2), (C.Structure,), {'_fields_': _fields(m.group(1), structs, constants)})
            continue
        params = [] if m.group(5).strip() == 'void' else m.group(5).split(',')
        args = []
        for p in params:
            a = re.fullmatch(r'(.*?[\s*])\w+\s*', p, re.S)
            if not a:
                raise ValueError(f'cannot split declarator: {p.strip()!r} of {m.group(4)}')
            args.append(_ctype(a.group(1), structs))
        functions[m.group(4)] = (_ctype(m.group(3), structs, ret=True), args)
    rest = re.sub(f'{_STRUCT}|{_PROTO}', '', text).split()
    if rest != ['}'] * n_extern:
        raise ValueError(f'not understood: {" ".join(rest)[:200]!r}')
    if len(functions) != n_functions or len(structs) != n_structs:
        raise ValueError(f'parsed {len(functions)} functions and {len(structs)} structs, the text names {n_functions} and {n_structs}')
    return constants, structs, functions
