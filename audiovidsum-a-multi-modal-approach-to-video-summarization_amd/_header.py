"""Reader of include/avsum_hip.h, the one description of libavsum_hip.so: its prototypes, its enumerators and integer
``#define``s, and the fields of its structs, with their ctypes.  _abi.py builds the binding from it and the host
table builders take the sizes they share with the kernels from it, so nothing of the header is typed a second time.

``re`` and ``ctypes`` only: importable without torch, numpy and the kernel library.  The reader knows the C the header
is written in and REFUSES everything else with a HeaderError that names the declaration - a header edit it cannot read
fails where the package is imported, not at a launch with shifted arguments."""
import ctypes
import functools
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "avsum_hip.h")

SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double,
           "size_t": ctypes.c_size_t, "unsigned": ctypes.c_uint, "uint32_t": ctypes.c_uint, "uint64_t": ctypes.c_uint64}
# what a pointer may point to (every pointer is passed as an address: c_void_p)
_POINTEES = set(SCALARS) | {"void", "char", "int32_t", "uint8_t", "uint16_t", "uint64_t"}

_INT = r"[-+]?(?:0[xX][0-9a-fA-F]+|\d+)"
_DECL = re.compile(r"((?:\w+\s+)*\w+)\s*(\**)\s*\b(\w+)")        # (type words) (stars) (name)


class HeaderError(ValueError):
    pass


def _one_line(text):
    return " ".join(text.split())


class Header:
    """``prototypes``: name -> (return type, [parameter types]); ``constants``: name -> int for every enumerator and
    every ``#define NAME <integer literal>``; ``structs``: name -> [(field, type)] of every ``typedef struct``.  Types
    are C spellings without ``const``, a pointer as ``"float*"``; ctype(), signatures() and fields() give their ctypes."""

    def __init__(self, text):
        self.prototypes, self.constants, self.structs, self._pointer_typedefs = {}, {}, {}, set()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        text = re.sub(r"\\\n", " ", text)
        for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(.*?)[ \t]*$", text, flags=re.M):
            if re.fullmatch(_INT, value):                      # (anything else is no shared number: not ours)
                self._constant(name, int(value, 0))
        text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
        if re.search(r'extern\s+"C"\s*\{', text):
            text, closed = re.subn(r"\}(?=[^}]*\Z)", " ", re.sub(r'extern\s+"C"\s*\{', " ", text, count=1), count=1)
            if not closed:
                raise HeaderError('extern "C" { is never closed')
        text = re.sub(r"\benum\s*\w*\s*\{([^{}]*)\}\s*;", self._enum, text)
        text = re.sub(r"\btypedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", self._struct, text)
        for statement in filter(None, map(_one_line, text.split(";"))):
            if statement.startswith("typedef "):
                self._typedef(statement)
            else:
                self._prototype(statement)

    def _constant(self, name, value):
        if self.constants.setdefault(name, value) != value:
            raise HeaderError(f"{name} is defined twice, as {self.constants[name]} and as {value}")

    def _enum(self, match):
        value = -1
        for item in filter(None, map(_one_line, match.group(1).split(","))):
            m = re.fullmatch(rf"(\w+)(?:\s*=\s*({_INT}))?", item)
            if not m:
                raise HeaderError(f"enumerator not understood: '{item}'")
            value = int(m.group(2), 0) if m.group(2) else value + 1
            self._constant(m.group(1), value)
        return " "

    def _declaration(self, text, where):
        """'const float* d_x' -> ('float*', 'd_x'); the type must be one ctype() maps."""
        m = _DECL.fullmatch(text)
        words = [w for w in m.group(1).split() if w != "const"] if m else []
        if len(words) != 1:
            raise HeaderError(f"{where}: declaration not understood: '{text}'")
        ctype = words[0] + m.group(2)
        self.ctype(ctype, where=where)
        return ctype, m.group(3)

    def _struct(self, match):
        name, fields = match.group(2), []
        for statement in filter(None, map(_one_line, match.group(1).split(";"))):
            first, *more = statement.split(",")
            ctype, field = self._declaration(first, f"struct {name}")
            for other in [field] + [_one_line(o) for o in more]:
                if not re.fullmatch(r"\w+", other):
                    raise HeaderError(f"struct {name}: declaration not understood: '{statement}'")
                fields.append((other, ctype))
        self.structs[name] = fields
        return " "

    def _typedef(self, statement):
        if not re.fullmatch(r"typedef void\s*\*\s*\w+", statement):
            raise HeaderError(f"typedef not understood: '{statement}'")
        self._pointer_typedefs.add(statement.split("*")[-1].strip())

    def _prototype(self, statement):
        m = re.fullmatch(r"(.*?)\b(\w+)\s*\((.*)\)", statement)
        if not m or not m.group(1).strip():
            raise HeaderError(f"prototype not understood: '{statement}'")
        name, params = m.group(2), m.group(3).strip()
        ret, _ = self._declaration(m.group(1) + name, f"{name}()")
        if name in self.prototypes:
            raise HeaderError(f"{name}() is declared twice")
        if not params:
            raise HeaderError(f"{name}(): an empty parameter list; write (void)")
        args = [] if params == "void" else [self._declaration(p.strip(), f"{name}()")[0] for p in params.split(",")]
        self.prototypes[name] = (ret, args)

    def ctype(self, c_type, returns=False, structs=None, where="type"):
        """The ctypes type of a C type.  Scalars by SCALARS; a ``char*`` RETURN is c_char_p; a pointer to a struct is
        POINTER(structs[name]) where ``structs`` gives its class; every other pointer - the pointer typedefs
        (avs_stream_t) among them - is c_void_p.  Everything else raises."""
        if c_type in SCALARS:
            return SCALARS[c_type]
        if c_type in self._pointer_typedefs:
            return ctypes.c_void_p
        base, stars = c_type.rstrip("*"), len(c_type) - len(c_type.rstrip("*"))
        if stars == 1 and base == "char" and returns:
            return ctypes.c_char_p
        if stars == 1 and base in self.structs:
            return ctypes.POINTER(structs[base]) if structs and base in structs else ctypes.c_void_p
        if stars == 1 and base in _POINTEES:
            return ctypes.c_void_p
        raise HeaderError(f"{where}: unknown type '{c_type}'")

    def fields(self, struct):
        """``_fields_`` of a ctypes.Structure for the header's ``struct``."""
        return [(field, self.ctype(c_type, where=f"struct {struct}")) for field, c_type in self.structs[struct]]

    def signatures(self, structs=None):
        """name -> (restype, [argtypes]) of every prototype; ``structs``: struct name -> its ctypes.Structure class."""
        return {name: (self.ctype(ret, True, structs, name), [self.ctype(a, False, structs, name) for a in args])
                for name, (ret, args) in self.prototypes.items()}


@functools.lru_cache(maxsize=None)
def load():
    """The package's own header, read and parsed once per process."""
    with open(HEADER_PATH) as f:
        return Header(f.read())
