"""ctypes binding of libullava_hip.so (the C-ABI declared in include/ullava_hip.h).

There is no fallback: if the library is missing or a symbol is absent this raises, and every op in
`ops.py` goes through here.  The library is built in-tree by `__graft_entry__.build()` /
`make -C u-llava_amd/csrc` so it travels with the repo snapshot.

The header is the one definition of the ABI.  It is parsed once, at import: every prototype becomes an entry of `SIGNATURES` (with its return
type in `RESTYPES`), the four `typedef struct` blocks become the ctypes classes below, and every `#define ULL_*` with an integer value lands in
`DEFINES`.  The C sources include the same header, so the compiler checks each definition against its declaration.  To add an entry point,
declare it in the header and define it in csrc/: nothing else needs a signature.
"""
import ast
import ctypes
import os
import re
from typing import NamedTuple

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ULL_LIB_PATH", os.path.join(_HERE, "csrc", "libullava_hip.so"))   # override: kernel A/B experiments only
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ullava_hip.h")

_SCALARS = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float}


class Header(NamedTuple):
    defines: dict       # macro name -> int
    structs: dict       # typedef name -> ctypes.Structure subclass
    signatures: dict    # entry point -> argtypes
    restypes: dict      # entry point -> restype


def _int_macro(body: str):
    """The value of a macro body made of integer literals, parentheses, `<<`, `|` and unary minus; None for anything else."""
    def ev(n):
        if isinstance(n, ast.Constant) and type(n.value) is int:
            return n.value
        if isinstance(n, ast.UnaryOp) and isinstance(n.op, ast.USub):
            return -ev(n.operand)
        if isinstance(n, ast.BinOp) and isinstance(n.op, (ast.LShift, ast.BitOr)):     # same precedence in C and in Python
            a, b = ev(n.left), ev(n.right)
            return a << b if isinstance(n.op, ast.LShift) else a | b
        raise ValueError(body)
    try:
        return ev(ast.parse(body.strip(), mode="eval").body)
    except (SyntaxError, ValueError):
        return None


def _ctype(base: str, pointer: bool, structs: dict, where: str):
    """int64_t / int / float, any pointer as void*, a known struct by value; anything else is an error, never a guess."""
    if pointer:
        return ctypes.c_void_p
    words = [w for w in base.split() if w != "const"]
    if len(words) == 1 and words[0] in _SCALARS:
        return _SCALARS[words[0]]
    if len(words) == 1 and words[0] in structs:
        return structs[words[0]]
    raise TypeError(f"u-llava_amd: {where}: no ctypes mapping for the C type `{base.strip()}`")


def _declarators(decl: str, where: str):
    """`const void *a, *b` / `int64_t n, k, ldw` / `const void* const* x` -> (base type, [(name, is pointer), ...])."""
    first, *more = [p.strip() for p in decl.split(",")]
    m = re.fullmatch(r"(.*?)(\w+)", first, flags=re.S)
    if not m or not m.group(1).strip():
        raise TypeError(f"u-llava_amd: {where}: cannot read the declaration `{decl.strip()}`")
    names = [(m.group(2), "*" in m.group(1))]
    for p in more:
        if not re.fullmatch(r"\**\s*\w+", p):
            raise TypeError(f"u-llava_amd: {where}: cannot read the declaration `{decl.strip()}`")
        names.append((p.lstrip("* "), "*" in p))
    return m.group(1).replace("*", " "), names


def parse_header(text: str) -> Header:
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    defines = {}
    for name, body in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(ULL_\w+)[ \t]+(\S.*?)[ \t]*$", text, flags=re.M):   # `NAME(` = function-like: no match
        value = _int_macro(body)
        if value is not None:
            defines[name] = value
    structs = {}
    for tag, body, name in re.findall(r"typedef\s+struct\s+(\w*)\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            base, names = _declarators(decl, name)
            fields += [(n, _ctype(base, ptr, structs, f"{name}.{n}")) for n, ptr in names]
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
    signatures, restypes = {}, {}
    for ret, name, params in re.findall(r"\b(int64_t|int)\s+(ull_\w+)\s*\(([^()]*)\)\s*;", text):
        args = []
        if params.split() != ["void"]:
            for i, p in enumerate(params.split(",")):
                where = f"{name}, parameter {i + 1}"
                base, ((_, pointer),) = _declarators(p, where)
                args.append(_ctype(base, pointer, {}, where))      # ({}: no struct travels by value in a call)
        signatures[name], restypes[name] = args, _SCALARS[ret]
    return Header(defines, structs, signatures, restypes)


_H = parse_header(open(HEADER_PATH).read())
DEFINES, SIGNATURES, RESTYPES = _H.defines, _H.signatures, _H.restypes      # restype: int = ULL_OK / ULL_ERR_*; int64_t = a plain query's answer

# the structs of the coarse entries (one call = a whole stack of layers)
Linear, LlamaLayer, ClipLayer, SamBlock = (_H.structs[n] for n in ("ull_linear", "ull_llama_layer", "ull_clip_layer", "ull_sam_block"))

WF_ELEM, WF_FP8, WF_MXFP4 = DEFINES["ULL_WF_ELEM"], DEFINES["ULL_WF_FP8"], DEFINES["ULL_WF_MXFP4"]   # the weight format of a Linear / of a *_wq_bf16 entry

ERRORS = {DEFINES["ULL_ERR_ARG"]: "ULL_ERR_ARG (null pointer / bad size)", DEFINES["ULL_ERR_SHAPE"]: "ULL_ERR_SHAPE (alignment or shape constraint)",
          DEFINES["ULL_ERR_LAUNCH"]: "ULL_ERR_LAUNCH (HIP launch failed)", DEFINES["ULL_ERR_LDS"]: "ULL_ERR_LDS (does not fit the LDS budget)"}

_lib = None


def load():
    """Load the shared library (once) and attach argtypes.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"u-llava_amd: HIP library not built: {LIB_PATH} is missing. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C u-llava_amd/csrc`. There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.argtypes = argtypes
        fn.restype = RESTYPES[name]
    _lib = lib
    return lib


def call(name: str, *args):
    fn = getattr(load(), name, None)
    if fn is None or name not in SIGNATURES:
        # (an op whose dtype has no kernel build: e.g. a backward / fused entry asked for float32 -- the fp32 build covers the inference path only)
        raise RuntimeError(f"u-llava_amd: the library has no entry point `{name}` (no kernel build of this op for that element type)")
    rc = fn(*args)
    if rc != 0:
        raise RuntimeError(f"u-llava_amd: {name} failed: {ERRORS.get(rc, rc)}")


def query(name: str, *args):
    """An entry point whose return value is the answer, not a status (int64_t in the header): returns its value."""
    fn = getattr(load(), name, None)
    if fn is None or name not in SIGNATURES:
        raise RuntimeError(f"u-llava_amd: the library has no entry point `{name}` (no kernel build of this op for that element type)")
    return fn(*args)
