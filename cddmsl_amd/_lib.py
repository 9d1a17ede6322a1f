"""ctypes binding of the C-ABI HIP library (``libcddmsl_hip.so``, declared in ``include/cddmsl_hip.h``).

The library is the product: every hot-path op of the package goes through it.  There is no CPU
or eager-PyTorch fallback -- if the shared object is missing, or a call returns a non-zero
status, this module raises.  PyTorch only supplies device memory (``Tensor.data_ptr()``) and the
stream handle the kernels are enqueued on.
"""
import ctypes
import os
import re

import torch  # noqa: F401  (must be imported first: it loads the HIP runtime the library binds to)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcddmsl_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "cddmsl_hip.h")
# the weight averaging of MODEL_EMA: a library and a header of its own, bound the same way
WEIGHT_AVERAGE_LIB_PATH = os.path.join(_HERE, "libcddmsl_weight_average.so")
WEIGHT_AVERAGE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "cddmsl_weight_average.h")

# the photometric augmentation of INPUT.COLOR_JITTER on the device path: likewise
COLOR_JITTER_LIB_PATH = os.path.join(_HERE, "libcddmsl_color_jitter.so")
COLOR_JITTER_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "cddmsl_color_jitter.h")

_lib = None
_lib_weight_average = None
_lib_color_jitter = None


class HipLibraryError(RuntimeError):
    pass


_BY_VALUE = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float}


def _statements(header_text):
    """The header's ``;``-terminated statements: comments, preprocessor lines and the ``extern "C"`` braces stripped."""
    text = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{|^\s*\}\s*$', " ", text, flags=re.M)
    return [" ".join(s.split()) for s in text.split(";") if s.strip()]


def header_signatures(header_text):
    """``{name: [ctypes type per parameter]}`` for every function the header declares.  Deliberately small and strict: a
    declaration is ``int cddmsl_<name>(<params>);``, a parameter is a pointer (any ``*``: ``c_void_p``, which takes ``ptr(t)``,
    None, ``byref`` and ctypes arrays alike) or a by-value ``int`` / ``long`` / ``float``.  Anything else raises."""
    sigs = {}
    for st in _statements(header_text):
        if "(" not in st:                           # no function: the members and the closing line of the struct typedef
            continue
        m = re.fullmatch(r"(.*?)\b(cddmsl_\w+) ?\((.*)\)", st)
        if m is None:
            raise HipLibraryError(f"include/cddmsl_hip.h: cannot parse the declaration `{st}`")
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        if ret != "int":
            raise HipLibraryError(f"include/cddmsl_hip.h: {name} returns `{ret}`; every entry point returns int")
        argtypes = []
        for p in ([] if params == "void" else params.split(",")):
            if "*" in p:
                argtypes.append(ctypes.c_void_p)
                continue
            words = [w for w in p.split() if w != "const"]
            if len(words) != 2 or words[0] not in _BY_VALUE:
                raise HipLibraryError(f"include/cddmsl_hip.h: {name}: parameter `{p.strip()}` is neither a pointer nor a "
                                      "by-value int / long / float")
            argtypes.append(_BY_VALUE[words[0]])
        sigs[name] = argtypes
    return sigs


def header_struct(header_text, name):
    """``[(member, ctypes type)]`` of ``typedef struct <name> { ... } <name>;`` in declaration order (int / long members only)."""
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S), flags=re.S)
    if m is None:
        raise HipLibraryError(f"include/cddmsl_hip.h: no struct {name}")
    fields = []
    for st in (s.split() for s in m.group(1).split(";") if s.strip()):
        if st[0] not in ("int", "long"):
            raise HipLibraryError(f"include/cddmsl_hip.h: struct {name}: unknown member type in `{' '.join(st)}`")
        fields += [(w.strip(","), _BY_VALUE[st[0]]) for w in st[1:]]
    return fields


def _load(lib_path, header_path):
    """Load a library and type every entry point from its header.  Raises if the library is not built or lacks a function the
    header declares; exports the header does not declare are left untyped."""
    if not os.path.exists(lib_path):
        raise HipLibraryError(
            f"{lib_path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  cddmsl_amd has no fallback path."
        )
    L = ctypes.CDLL(lib_path)
    with open(header_path) as f:
        sigs = header_signatures(f.read())
    for name, argtypes in sigs.items():
        fn = getattr(L, name, None)
        if fn is None:
            raise HipLibraryError(f"{lib_path} is stale: it does not export {name}, which include/{os.path.basename(header_path)} declares; rebuild it")
        fn.restype, fn.argtypes = ctypes.c_int, argtypes
    return L


def lib():
    """Return the loaded library, loading it on first use, every entry point typed from include/cddmsl_hip.h."""
    global _lib
    if _lib is None:
        _lib = _load(LIB_PATH, HEADER_PATH)
    return _lib


def lib_weight_average():
    """libcddmsl_weight_average.so (csrc/weight_average.hip), typed from include/cddmsl_weight_average.h; loaded on first use."""
    global _lib_weight_average
    if _lib_weight_average is None:
        _lib_weight_average = _load(WEIGHT_AVERAGE_LIB_PATH, WEIGHT_AVERAGE_HEADER_PATH)
    return _lib_weight_average


def lib_color_jitter():
    """libcddmsl_color_jitter.so (csrc/color_jitter.hip), typed from include/cddmsl_color_jitter.h; loaded on first use."""
    global _lib_color_jitter
    if _lib_color_jitter is None:
        _lib_color_jitter = _load(COLOR_JITTER_LIB_PATH, COLOR_JITTER_HEADER_PATH)
    return _lib_color_jitter


def stream_ptr():
    """The HIP stream torch is currently enqueuing on, as a void* (raw-stream query: ~1 us, this runs once per launch)."""
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


def to_device_async(cpu_tensor, device):
    """Host -> device copy that does NOT synchronise: staged through pinned memory and enqueued on the current stream
    (a pageable ``.to(device)`` blocks until everything already queued has run, i.e. acts as a full device sync)."""
    if torch.device(device).type == "cpu":
        return cpu_tensor
    if cpu_tensor.numel() == 0:
        return torch.empty(cpu_tensor.shape, dtype=cpu_tensor.dtype, device=device)
    return cpu_tensor.pin_memory().to(device, non_blocking=True)


def ptr(t):
    """Device pointer of a tensor (or NULL for None)."""
    if t is None:
        return ctypes.c_void_p(0)
    return ctypes.c_void_p(t.data_ptr())


def check(status, what):
    if status != 0:
        raise HipLibraryError(f"{what} failed with status {status}")


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise HipLibraryError(
                "cddmsl_amd ops run only on the MI355X HIP path; got a CPU tensor "
                "(the CPU restatement lives in oracle/ and is test infrastructure only)"
            )


class Readback:
    """Device -> host copy whose wait covers ONLY the work enqueued before it: the copy goes to pinned memory on the current
    stream and an event is recorded right behind it; ``get()`` blocks on that event.  A ``tensor.cpu()`` / ``.tolist()`` at the
    point of use would instead wait for everything enqueued in between -- the idea here is to enqueue independent device work
    (the next stage, another branch) between issuing a readback and consuming it, so the device stays busy while the host
    does the data-dependent part (sampling permutations, list building)."""

    def __init__(self, t):
        if t.is_cuda:
            self.host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            self.host.copy_(t, non_blocking=True)
            self.ev = torch.cuda.Event()
            self.ev.record()
        else:
            self.host, self.ev = t, None

    def get(self):
        if self.ev is not None:
            self.ev.synchronize()
        return self.host
