"""A reader of the C declarations in include/srk.h: the one source of the ctypes binding (_lib.py).

read(text) takes the header's text and returns a Header with
  constants  {name: int}       every `#define SRK_X <integer>` and every enumerator (an alias takes its target's value)
  structs    {name: [(field, ctype)]}   every `typedef struct ... srk_x`, fields in order
  classes    {name: ctypes.Structure subclass made of those fields}
  functions  {name: (restype, [argtypes])}   every function declaration
  spellings  {name: (return type, [parameter types])}   the same declarations as C text, parameter names removed

How a C type becomes a ctype: a by-value scalar maps to its fixed ctype (SCALARS); `const char*` as a return type is
c_char_p; a pointer to an srk_ struct is POINTER(its class); EVERY other pointer is c_void_p -- pointers to scalars,
void*, const float* const*, the stream.  The header does not say whether a `const int64_t*` is a host array or a device
pointer, and ctypes rejects a c_void_p instance where it is told POINTER(c_int64); c_void_p takes everything a caller
has: a c_void_p, None, a ctypes array, a data_as() result, byref().

The header is regular, and the reader holds it to that: an unknown type name, a function pointer, a bit-field, an array
parameter, a struct passed by value, an enumerator without a value, nested braces, a macro that is not an integer all
raise a RuntimeError that names the declaration.  Nothing is skipped or guessed.
"""
import collections
import ctypes
import re

SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
           "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double,
           "long long": ctypes.c_longlong}
POINTEES = set(SCALARS) | {"void", "char", "uint8_t"}   # what a pointer may point at

Header = collections.namedtuple("Header", "constants structs classes functions spellings")

_INT = r"[-+]?(?:0[xX][0-9a-fA-F]+|\d+)"


def _fail(decl, why):
    raise RuntimeError("include/srk.h: %s in `%s`" % (why, " ".join(decl.split())))


def _split_type(decl, text, structs, named):
    """`const float* const* x` -> ("float", 2, "const float * const *", "x"): base type, pointer depth, C spelling, name."""
    if re.search(r"[^\w\s*]", text):
        _fail(decl, "%s is not a plain type (function pointer, array, bit-field or initialiser)" % " ".join(text.split()))
    tokens = re.findall(r"\w+|\*", text)
    words = [t for t in tokens if t not in ("*", "const")]
    name = None
    if " ".join(words) not in POINTEES and " ".join(words) not in structs:
        if len(words) < 2 or tokens[-1] != words[-1]:
            _fail(decl, "unknown type `%s`" % " ".join(words))
        name = words.pop()
        tokens = tokens[:-1]
    if named and name is None:
        _fail(decl, "no name after type `%s`" % " ".join(words))
    base = " ".join(words)
    if base not in POINTEES and base not in structs:
        _fail(decl, "unknown type `%s`" % base)
    return base, tokens.count("*"), " ".join(tokens), name


def _ctype(decl, base, stars, classes, is_return=False):
    if stars == 0:
        if base in classes:
            _fail(decl, "struct %s by value" % base)
        if base not in SCALARS:
            _fail(decl, "`%s` by value" % base)
        return SCALARS[base]
    if is_return:
        if (base, stars) != ("char", 1):
            _fail(decl, "pointer return type other than const char*")
        return ctypes.c_char_p
    if base in classes and stars == 1:
        return ctypes.POINTER(classes[base])
    return ctypes.c_void_p


def _constant(decl, value, constants):
    value = value.strip()
    if re.fullmatch(_INT, value):
        return int(value, 0)
    if value in constants:
        return constants[value]
    _fail(decl, "value `%s` is neither an integer nor an earlier constant" % value)


def _enum(decl, body, constants):
    for item in body.split(","):
        if not item.strip():
            continue
        name, eq, value = item.partition("=")
        if not eq or not re.fullmatch(r"\w+", name.strip()):
            _fail(decl, "enumerator `%s` without a value" % " ".join(item.split()))
        constants[name.strip()] = _constant(decl, value, constants)


def _struct(decl, body, structs, classes):
    fields = []
    for member in body.split(";"):
        if not member.strip():
            continue
        first, *more = member.split(",")
        array = re.fullmatch(r"(.*?)\[\s*(\d+)\s*\]\s*", first, flags=re.S)
        base, stars, _, name = _split_type(decl, array.group(1) if array else first, structs, named=True)
        if array and (more or (base, stars) != ("char", 0)):
            _fail(decl, "array field other than one `char name[N]`")
        ctype = ctypes.c_char * int(array.group(2)) if array else _ctype(decl, base, stars, {})
        fields.append((name, ctype))
        for extra in more:                       # `int32_t N, H, W, Cin;`: more names of the same type
            if not re.fullmatch(r"\s*[A-Za-z_]\w*\s*", extra):
                _fail(decl, "`%s` is not a plain field name" % " ".join(extra.split()))
            fields.append((extra.strip(), ctype))
    return fields


def _function(decl, structs, classes):
    m = re.fullmatch(r"\s*([^()]*?)\(([^()]*)\)\s*", decl, flags=re.S)
    if not m:
        _fail(decl, "not a function declaration (function pointer or nested parentheses)")
    base, stars, ret, name = _split_type(decl, m.group(1), structs, named=True)
    restype = _ctype(decl, base, stars, classes, is_return=True)
    argtypes, params = [], []
    if m.group(2).strip() != "void":
        for p in m.group(2).split(","):
            base, stars, spelled, _ = _split_type(decl, p, structs, named=False)
            if base == "void" and stars == 0:
                _fail(decl, "parameter of type void")
            argtypes.append(_ctype(decl, base, stars, classes))
            params.append(spelled)
    return name, (restype, argtypes), (ret, params)


def read(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b[^\n]*", " ", text, flags=re.S | re.M)
    constants, structs, classes, functions, spellings = {}, {}, {}, {}, {}
    lines = []
    for line in text.split("\n"):
        if not line.lstrip().startswith("#"):
            lines.append(line)
            continue
        m = re.fullmatch(r"\s*#\s*define\s+(\w+)\s*(.*?)\s*", line)
        if m and m.group(2):
            constants[m.group(1)] = _constant(line, m.group(2), constants)
        elif not m and not re.match(r"\s*#\s*(include|ifndef|endif)\b", line):
            _fail(line, "preprocessor line the reader does not know")
    for decl in re.findall(r"(?:[^;{}]|\{[^{}]*\})+;|[^;]+", "\n".join(lines)):
        decl = decl.strip().rstrip(";")
        if not decl:
            continue
        m = re.fullmatch(r"(typedef\s+)?(enum|struct)\s*(\w*)\s*\{([^{}]*)\}\s*(\w*)\s*", decl, flags=re.S)
        if m is None:
            if "{" in decl or "}" in decl or re.match(r"(typedef|enum|struct)\b", decl):
                _fail(decl, "nested braces or a typedef the reader does not know")
            name, functions[name], spellings[name] = _function(decl, structs, classes)
        elif m.group(2) == "enum":
            _enum(decl, m.group(4), constants)
        elif not (m.group(1) and m.group(5)):
            _fail(decl, "struct without a typedef name")
        else:
            structs[m.group(5)] = _struct(decl, m.group(4), structs, classes)
            classes[m.group(5)] = type(m.group(5), (ctypes.Structure,), {"_fields_": structs[m.group(5)]})
    for name in list(constants) + list(structs) + list(functions):
        if not name.lower().startswith("srk_"):
            _fail(name, "a name outside the library's SRK_ / srk_ prefix")
    return Header(constants, structs, classes, functions, spellings)


def read_file(path):
    try:
        with open(path) as f:
            text = f.read()
    except OSError as e:
        raise RuntimeError("cannot read the C ABI header %s (%s): the binding is derived from it" % (path, e))
    return read(text)
