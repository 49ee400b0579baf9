"""ctypes binding of csrc/liblidar_hip.so — the only way the Python host side reaches the kernels.

Deliberately no fallback: if the shared library is missing or a symbol is absent we raise, so a
silent eager/PyTorch path can never stand in for the HIP path.
"""
import ast
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("LIDAR_HIP_SO") or os.path.join(_HERE, "csrc", "liblidar_hip.so")   # env override: A/B builds (tools/)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "lidar_hip.h")


class LidarHipError(RuntimeError):
    pass


# by-value C types of the ABI; a pointer to any of them, of any depth and constness, is a c_void_p
_CTYPES = {"void": None, "int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "long long": C.c_longlong,
           "char": C.c_char, "signed char": C.c_byte, "unsigned char": C.c_ubyte, "unsigned": C.c_uint, "unsigned int": C.c_uint,
           "unsigned long long": C.c_ulonglong, "uint32_t": C.c_uint32, "int64_t": C.c_int64}
_QUALIFIERS = {"const", "volatile", "restrict", "__restrict__"}
_INT_OPS = {ast.LShift: int.__lshift__, ast.Mult: int.__mul__, ast.Add: int.__add__}


def _ctype(text, decl, named):
    """ctypes of one parameter (`named`: an identifier may follow the type) or of a return type, as written in C"""
    if "[" in text:
        raise LidarHipError(f"{decl}: array parameter `{text.strip()}`")
    tok = [t for t in re.findall(r"\w+|\S", text) if t not in _QUALIFIERS]
    pointer = "*" in tok
    base = tok[:tok.index("*")] if pointer else tok
    rest = [t for t in tok[len(base):] if t != "*"]                     # behind the stars: nothing, or the parameter's name
    if not pointer and named and len(base) > 1 and " ".join(base) not in _CTYPES:
        base, rest = base[:-1], base[-1:]
    if len(rest) > named or not all(re.fullmatch(r"[A-Za-z_]\w*", t) for t in rest):
        raise LidarHipError(f"{decl}: cannot read `{text.strip()}`")
    name = " ".join(base)
    if name not in _CTYPES or (named and not pointer and name == "void"):
        what = "by-value struct" if not pointer and base[:1] in (["struct"], ["union"]) else "unknown base type"
        raise LidarHipError(f"{decl}: {what} `{name}` in `{text.strip()}`")
    return C.c_void_p if pointer else _CTYPES[name]


def _int_expr(text, name):
    """value of a constant expression of integer literals (decimal / hex, u / l / ll suffixes), parentheses, unary minus, `<<`, `*`
    and `+`.  Python's grammar gives these the precedence C does; only these node kinds are evaluated, nothing is eval()ed"""
    def value(n):
        if isinstance(n, ast.Constant) and type(n.value) is int:
            return n.value
        if isinstance(n, ast.UnaryOp) and isinstance(n.op, ast.USub):
            return -value(n.operand)
        if isinstance(n, ast.BinOp) and type(n.op) in _INT_OPS:
            return _INT_OPS[type(n.op)](value(n.left), value(n.right))
        raise ValueError(n)
    try:
        return value(ast.parse(re.sub(r"\b(0[xX][0-9a-fA-F]+|\d+)[uUlL]+\b", r"\1", text), mode="eval").body)
    except (SyntaxError, ValueError):
        raise LidarHipError(f"#define {name}: `{text}` is not an integer expression this parser reads") from None


def parse_header(text):
    """include/lidar_hip.h -> (signatures, limits): signatures[name] = (restype, argtypes) of every function the header declares,
    limits[name] = value of every object-like `#define LIDAR_<NAME> <integer expression>`.  Strict: what it cannot map exactly
    (an unknown type, a struct by value, an array or function-pointer parameter, a variadic list, two differing declarations of
    one name) raises LidarHipError naming the declaration."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S).replace("\\\n", " ")
    signatures, limits, code = {}, {}, []
    for line in text.split("\n"):
        if not line.lstrip().startswith("#"):
            code.append(line)
            continue
        m = re.match(r"\s*#\s*define\s+(LIDAR_\w+)(?!\()\s+(\S.*)", line)     # not function-like, not the bare include guard
        value = m and _int_expr(m.group(2).strip(), m.group(1))
        if m and limits.setdefault(m.group(1), value) != value:
            raise LidarHipError(f"#define {m.group(1)}: defined twice with different values")
    for decl in re.sub(r'extern\s+"C"\s*\{|^\s*\}', " ", "\n".join(code), flags=re.M).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.fullmatch(r"(.*?)\b([A-Za-z_]\w*)\s*\((.*)\)", decl)
        if not m or not m.group(1).strip():
            raise LidarHipError(f"cannot read the declaration `{decl}`")
        ret, name, args = m.group(1), m.group(2), m.group(3).strip()
        for mark, what in (("...", "variadic parameter list"), ("(", "function-pointer parameter")):
            if mark in args:
                raise LidarHipError(f"{name}: {what}")
        if not args:
            raise LidarHipError(f"{name}: empty parameter list; write (void)")
        sig = (_ctype(ret, name, False), [] if args == "void" else [_ctype(a, name, True) for a in args.split(",")])
        if signatures.setdefault(name, sig) != sig:
            raise LidarHipError(f"{name}: declared twice with different types")
    return signatures, limits


if not os.path.exists(HEADER_PATH):
    raise LidarHipError(f"{HEADER_PATH} is missing: the ctypes signatures and the LIDAR_* limits are read from it; there is no second copy")
with open(HEADER_PATH) as _f:
    # name -> (restype, argtypes) of every function the header declares, and name -> value of its LIDAR_* constants
    SIGNATURES, LIMITS = parse_header(_f.read())

_lib = None


def _bind(path):
    """load the library at `path` and give every declared function its types"""
    so = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(so, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    return so


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise LidarHipError(
                f"{SO_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        _lib = _bind(SO_PATH)
    return _lib


def load_variant(path):
    """A second, independently loaded build of the library with the same signatures (tests: A/B variants from
    csrc/build.py:VARIANTS).  The product path never calls this."""
    if not os.path.exists(path):
        raise LidarHipError(f"{path} is missing: build it with lidardetection_amd/csrc/build.py (build_variants)")
    return _bind(path)


def check(status, what):
    if status != 0:
        raise LidarHipError(f"{what} failed with status {status}")


def fail(what, msg):
    """refuse an argument of the wrapper `what`"""
    raise LidarHipError(f"{what}: {msg}")


def cfg_get(cfg, key, default=None):
    """an entry of a model config, which is a dict (EasyDict) in the reference and may be a plain namespace in tests"""
    return cfg.get(key, default) if hasattr(cfg, "get") else getattr(cfg, key, default)


def ptr(t):
    """device (or host) address of a torch tensor / None."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    """Raw hipStream_t of torch's current stream on the current device (the private fast accessors avoid the
    ~0.1 ms torch.cuda.current_stream() spends in availability checks on every call)."""
    import torch
    try:
        return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))
    except AttributeError:  # pragma: no cover - older/newer torch without the private accessors
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def host_f32(vals):
    return (C.c_float * len(vals))(*[float(v) for v in vals])


def host_i32(vals):
    return (C.c_int * len(vals))(*[int(v) for v in vals])


def require_cuda(*tensors, allow=()):
    """Every tensor handed to the C ABI: on the device, contiguous, and float32 or int32 (the only element types the kernels
    read; the reference assumes them without checking — a float64 / int64 tensor would be reinterpreted bit-wise).  `allow`:
    further dtypes a particular entry point takes (e.g. torch.int64 keep lists)."""
    import torch
    ok = (torch.float32, torch.int32) + tuple(allow)
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise LidarHipError("expected a CUDA (ROCm) tensor; this library has no CPU path")
        if not t.is_contiguous():
            raise LidarHipError("expected a contiguous tensor")
        if t.dtype not in ok:
            raise LidarHipError(f"expected a float32 / int32 tensor, got {t.dtype} (shape {tuple(t.shape)})")


def require_nhwc(x, what):
    """a kernel's input map: a fully contiguous channels-last (B, C, H, W) float32 tensor on the device"""
    import torch
    if not (x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)):
        raise LidarHipError(f"{what}: expected a channels-last float32 CUDA tensor")


def nhwc_ld(t, what):
    """-> row stride (floats) of a channels-last (B, C, H, W) fp32 CUDA map or of a channel slice of one"""
    import torch
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 4):
        raise LidarHipError(f"{what}: expected a 4-d float32 CUDA (ROCm) tensor, got {t.dtype} {tuple(t.shape)} on {t.device}")
    B, Cc, H, W = t.shape
    ld = t.stride(3)
    if t.stride() != (H * W * ld, 1, W * ld, ld) or ld < Cc:
        raise LidarHipError(f"{what}: expected a channels-last map (or a channel slice of one), got strides {t.stride()}")
    return ld


def nhwc_out(what, B, hw, cout, device, out=None, out_offset=0, sliced=False):
    """where a kernel writes its `cout` channels for a map of batch B and spatial shape hw: -> (out, out_offset).  out=None: a new
    channels-last float32 (B, cout, *hw) map, offset 0.  Otherwise `out`, checked: a fully contiguous channels-last float32 CUDA map
    (sliced=True: or a channel slice of one, nhwc_ld) of that batch and spatial shape with channels [out_offset, out_offset + cout)."""
    import torch
    if out is None:
        return torch.empty((B, cout, *hw), dtype=torch.float32, device=device, memory_format=torch.channels_last), 0
    if sliced:
        nhwc_ld(out, what + " out")
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous(memory_format=torch.channels_last)):
        raise LidarHipError(f"{what}: output must be a channels-last float32 CUDA tensor")
    if out.shape[0] != B or tuple(out.shape[2:]) != tuple(hw) or not 0 <= out_offset <= out.shape[1] - cout:
        raise LidarHipError(f"{what}: output must be ({B}, >= out_offset + {cout}, *{tuple(hw)}), got {tuple(out.shape)} with out_offset {out_offset}")
    return out, out_offset


def require_last(t, k, what):
    """last dimension of `t` must be k (boxes: 7, points: 3, ...)"""
    if t is not None and (t.dim() == 0 or t.shape[-1] != k):
        raise LidarHipError(f"{what}: expected (..., {k}), got {tuple(t.shape)}")
