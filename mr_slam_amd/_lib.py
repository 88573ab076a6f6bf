"""ctypes binding of libmrslam_hip.so, typed from its C ABI header (include/mrslam_hip.h).

load() reads the header's prototypes and binds every `mrs_*` function once.  A bound function checks its argument count and
every pointer argument (placement from the parameter's `d_` / `h_` prefix, element type from its declared type) before C is
called, and turns a non-zero status into MrsError.  There is no CPU fallback: if the shared library is missing or no GPU is
visible the product path raises.  PyTorch is used only for device memory and streams.
"""
import ctypes as C
import os
import re
import sys
import threading
import types

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmrslam_hip.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "mrslam_hip.h")

MRS_OK = 0
OUT_REFERENCE = 0
OUT_COMPACT = 1
DROPPED = -2**31

# the int functions whose return value is a value, not a status (plus the void / double / const char* ones)
VALUE_RETURNING = ("mrs_abi_version", "mrs_ctx_device", "mrs_exchange_available", "mrs_gicp_batch_last_nn_passes",
                   "mrs_gicp_batch_last_searched_fraction", "mrs_status_str", "mrs_last_error", "mrs_gicp_default_params", "mrs_icp_default_params",
                   "mrs_pclgicp_default_params", "mrs_icp_plane_default_params")


class MrsError(RuntimeError):
    def __init__(self, msg, status=None):
        super().__init__(msg)
        self.status = status


class BevCfg(C.Structure):
    _fields_ = [("max_length", C.c_int32), ("max_height", C.c_int32), ("n0", C.c_int32),
                ("n1", C.c_int32), ("num_height", C.c_int32), ("enough_large", C.c_int32)]


_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
_RESTYPES = {"int": C.c_int32, "double": C.c_double, "char*": C.c_char_p, "void": None}
_ELEMENTS = {"float": ("float32", "complex64"), "double": ("float64", "complex128"), "int32_t": ("int32",),
             "int64_t": ("int64",), "uint8_t": ("uint8",), "uint64_t": ("uint64",)}      # void and the opaque types take any element type


_header_text = {}


def _header(path=None):
    """the text of a header (HEADER when None), read once per process"""
    path = path or HEADER
    if path not in _header_text:
        _header_text[path] = open(path).read()
    return _header_text[path]


def header_int(name):
    """the integer of `#define name <int>` in the C ABI header"""
    m = re.search(r"#define\s+%s\s+(\d+)" % re.escape(name), _header())
    if m is None:
        raise MrsError("%s does not define %s" % (HEADER, name))
    return int(m[1])


def parse_header(path):
    """{name: (return type, [(type, pointer depth, parameter name), ...])} of every `mrs_*` declaration in the header"""
    src = re.sub(r"/\*.*?\*/|//[^\n]*", "", _header(path), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"^\s*(?:const\s+)?(\w+\s*\**)\s*(mrs_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        args = []
        for p in params.split(","):
            m = re.fullmatch(r"\s*(?:const\s+)?(\w+)((?:\s*\*(?:\s*const\b)?)*)\s*\b(\w+)\s*", p)
            if m:
                args.append((m[1], m[2].count("*"), m[3]))
            elif p.strip() != "void":
                raise MrsError("%s: cannot parse parameter %r of %s" % (path, p.strip(), name))
        protos[name] = (ret.replace(" ", ""), args)
    return protos


_TENSOR, _ARRAY, _PASS = 1, 2, 3
_kinds = {type(None): _PASS}           # by exact type: what a pointer slot does with a value of that type
_CTYPES = (C._SimpleCData, C.Array, C._Pointer, C._CFuncPtr, type(C.byref(C.c_int())))
_dtype_names = {}


def _kind(tp):
    torch = sys.modules.get("torch")   # no tensor exists before torch is imported
    for k, base in ((_TENSOR, torch.Tensor if torch else ()), (_ARRAY, np.ndarray), (_PASS, _CTYPES)):
        if issubclass(tp, base):
            _kinds[tp] = k
            return k
    return None


def _address(fn, param, on_device, dtypes, x):
    """checked address of a tensor / array passed for pointer parameter `param` (the slow path of a bound call)"""
    k = _kinds.get(type(x)) or _kind(type(x))
    if k is _PASS:
        return x
    if k is None:
        raise TypeError("%s: %s: expected a tensor, an array, None or a ctypes object, got %s" % (fn, param, type(x).__name__))
    if on_device is not None and (k is _TENSOR and x.is_cuda) is not on_device:
        raise MrsError("%s: %s: expected a %s" % (fn, param, "device tensor (no CPU fallback)" if on_device else "host tensor or array"))
    dt = _dtype_names.get(x.dtype) or _dtype_names.setdefault(x.dtype, str(x.dtype).replace("torch.", ""))
    if dtypes is not None and dt not in dtypes:
        raise TypeError("%s: %s: element type %s, expected %s" % (fn, param, dt, " or ".join(dtypes) or "a ctypes object"))
    return x.data_ptr() if k is _TENSOR else x.ctypes.data


def _bind(cdll, name, ret, params):
    if not hasattr(cdll, name):
        raise MrsError("%s does not export %s, which %s declares: rebuild it" % (LIB_PATH, name, HEADER))
    cfn = getattr(cdll, name)
    pointer = [bool(depth) or base == "mrs_stream" for base, depth, _ in params]
    try:
        cfn.restype = _RESTYPES[ret]
        cfn.argtypes = [C.c_void_p if ptr else _SCALARS[base] for ptr, (base, _, _) in zip(pointer, params)]
    except KeyError:
        raise MrsError("%s: unsupported type in the declaration of %s" % (HEADER, name)) from None
    # pointer slots: (index, name, placement from the d_ / h_ prefix, element types; () = ctypes objects only: pointers to pointers, streams)
    slots = [(i, p, {"d_": True, "h_": False}.get(p[:2]), _ELEMENTS.get(base) if depth == 1 else ())
             for i, (ptr, (base, depth, p)) in enumerate(zip(pointer, params)) if ptr]
    n, status = len(params), name not in VALUE_RETURNING

    def call(*args):
        if len(args) != n:
            raise TypeError("%s takes %d arguments (%d given)" % (name, n, len(args)))
        args = list(args)
        for i, param, on_device, dtypes in slots:
            x = args[i]
            k = _kinds.get(type(x))
            if k is _PASS:
                continue
            if k is _TENSOR and (on_device is None or x.is_cuda is on_device) and (dtypes is None or _dtype_names.get(x.dtype) in dtypes):
                args[i] = x.data_ptr()
            elif k is _ARRAY and not on_device and (dtypes is None or _dtype_names.get(x.dtype) in dtypes):
                try:                # a third of the cost of x.ctypes.data; needs a writable, non-empty, contiguous array
                    args[i] = C.addressof(C.c_char.from_buffer(x))
                except (TypeError, ValueError, BufferError):
                    args[i] = x.ctypes.data
            else:                   # first sight of a type or dtype, or a rejected value
                args[i] = _address(name, param, on_device, dtypes, x)
        try:
            r = cfn(*args)
        except C.ArgumentError as e:
            raise TypeError("%s: %s" % (name, e)) from None
        if status and r:
            raise MrsError("%s: %s" % (_status_str(r).decode(), _last_error().decode()), r)
        return r
    call.__name__ = name
    return call


_lib = None
_status_str = _last_error = None
_lock = threading.Lock()
_ctx = {}


def load():
    """The bound C ABI (one attribute per header function); raises MrsError (never falls back) if the library is not built,
    lacks a declared function or was built against another ABI version."""
    global _lib, _status_str, _last_error
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise MrsError(
                        f"{LIB_PATH} not found: build it with `make -C mr_slam_amd/csrc` "
                        "(or __graft_entry__.build()); there is no CPU fallback")
                if not os.path.exists(HEADER):
                    raise MrsError(f"{HEADER} not found: the binding takes its prototypes from it")
                cdll = C.CDLL(LIB_PATH)
                api = types.SimpleNamespace(**{n: _bind(cdll, n, r, p) for n, (r, p) in parse_header(HEADER).items()})
                _status_str, _last_error = cdll.mrs_status_str, cdll.mrs_last_error
                want = header_int("MRS_ABI_VERSION")
                if api.mrs_abi_version() != want:
                    raise MrsError("%s has ABI version %d, %s declares %d: rebuild it" % (LIB_PATH, api.mrs_abi_version(), HEADER, want))
                _lib = api
    return _lib


def ctx(device=0):
    """Per-process, per-device context handle (created on first use)."""
    lib = load()
    with _lock:
        h = _ctx.get(device)
        if h is None:
            h = C.c_void_p()
            lib.mrs_ctx_create(int(device), C.byref(h))
            _ctx[device] = h
    return h


def device_of(t):
    """Device index of a tensor the product path runs on; there is no CPU fallback."""
    if not getattr(t, "is_cuda", False):
        raise MrsError("expected a device tensor (no CPU fallback)")
    return t.device.index or 0


def current_stream(device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Handle:
    """Owner of one C handle: `_h` is a plain c_void_p to pass to the C ABI; a subclass names its destroy function in `_destroy` and opens
    with `self._create("mrs_x_create", ...)`."""
    _destroy = None

    def _create(self, fn_name, *args):
        self._h = C.c_void_p()               # before the call: a create that raises leaves a null handle, which __del__ skips
        getattr(load(), fn_name)(*args, C.byref(self._h))

    def __del__(self):
        try:                                 # silent: at interpreter shutdown the library or this module may be gone already
            h = getattr(self, "_h", None)
            if h:
                self._h = None
                getattr(load(), self._destroy)(h)
        except Exception:
            pass


def in_range(name, value, hi):
    """int(value) if 1 <= value <= hi, else ValueError("<name> in 1..<hi>")"""
    value = int(value)
    if not 1 <= value <= hi:
        raise ValueError("%s in 1..%d" % (name, hi))
    return value


def ragged(points, offsets, *, dtype=None, exact=False):
    """The leading arguments of a ragged-batch call: packed points [N, stride >= 3] on the device, cloud b = points[offsets[b]:offsets[b + 1]].
    -> (device index, contiguous points, (h_off, d_off, B)) with int64 offsets on the host and on the points' device.
    offsets: a tensor on either side, an array or a list (copied to the side it is not on), or a (host, device) pair of tensors, used as
    it is.  dtype: the points are cast to it; None keeps float32 / float64 and widens anything else to float64.  The last offset may
    stay below N unless exact, which also wants the first to be 0."""
    import torch
    d = device_of(points)
    p = points.detach()
    assert p.dim() == 2 and p.shape[1] >= 3, tuple(p.shape)
    if dtype is not None:
        p = p.to(dtype)
    elif p.dtype not in (torch.float32, torch.float64):
        p = p.to(torch.float64)
    p = p.contiguous()
    if isinstance(offsets, (tuple, list)) and len(offsets) == 2 and isinstance(offsets[0], torch.Tensor):
        h_off, d_off = offsets
    else:
        h_off = d_off = offsets if isinstance(offsets, torch.Tensor) else torch.as_tensor(np.asarray(offsets, np.int64))
    h_off = h_off.detach().to("cpu", torch.int64).contiguous()
    d_off = d_off.detach().to(p.device, torch.int64).contiguous()
    B, last = h_off.numel() - 1, int(h_off[-1])
    if exact:
        assert B >= 1 and int(h_off[0]) == 0 and last == p.shape[0], (h_off.tolist()[:4], p.shape[0])
    else:
        assert B >= 1 and last <= p.shape[0], (B, last, p.shape[0])
    return d, p, (h_off, d_off, B)


def one_cloud(cloud, device):
    """one cloud [n, >= 3] of any origin (device tensor, host tensor or array) -> ([n, s] device tensor, host offsets [0, n])"""
    import torch
    if not isinstance(cloud, torch.Tensor):
        cloud = torch.from_numpy(np.ascontiguousarray(cloud))
    if not cloud.is_cuda:
        cloud = cloud.to(device)
    cloud = cloud.reshape(-1, cloud.shape[-1] if cloud.dim() == 2 else 3)
    return cloud, torch.tensor([0, cloud.shape[0]], dtype=torch.int64)
