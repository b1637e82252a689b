"""ctypes binding of libslamhip.so (include/slam_hip.h).

This is the binding a maintainer of the reference would add next to
course_agv_slam/scripts: the reference has no FFI layer of its own, so
the C ABI is bound here one function per reference method.

The library is the ONLY implementation of the hot path: there is no CPU fallback.  If the
shared object is missing, or no gfx950 device is visible when a context is created, the
package raises instead of computing anything on the host.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import re
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SLAM_HIP_LIB") or os.path.join(_HERE, "libslamhip.so")   # override: A/B builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "slam_hip.h")
REFINE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "slam_refine.h")     # the second header: slam_grid_refine(_dev)
TRACK_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "slam_track.h")       # the third header: slam_track(_dev)

SLAM_OK, ERR_INVALID, ERR_HIP, ERR_NOMEM, ERR_NAN, ERR_OVERFLOW, ERR_NODEVICE = 0, -1, -2, -3, -4, -5, -6
F64, F32, F16 = 0, 1, 2
DTYPES = {"f64": F64, "f32": F32, "f16": F16, np.float64: F64, np.float32: F32, np.float16: F16}
NP_DTYPES = {F64: np.float64, F32: np.float32, F16: np.float16}
K_NAMES = ("points", "icp", "compose", "grid", "finalize", "nn", "kabsch", "bresenham")


class SlamError(RuntimeError):
    """A libslamhip call failed (bad argument, HIP error, no device)."""


class LibraryMissing(ImportError):
    """libslamhip.so has not been built; there is no fallback implementation."""


_lib = None
_lib_lock = threading.Lock()

_vp = C.c_void_p
_BY_VALUE = {"int": C.c_int, "double": C.c_double, "float": C.c_float, "int64_t": C.c_int64}


def _ctype(decl, text):
    """The ctypes type of one parameter or return type ``text`` of declaration ``decl``: ``int``, ``double``, ``float``
    and ``int64_t`` by value, ``char *`` a ``c_char_p``, every other pointer or array a void pointer.  Anything else
    raises: a width this binding does not know must not be passed as an ``int``."""
    words = re.sub(r"\bconst\b", " ", text.replace("*", " * ")).split()
    if "*" in text or "[" in text:
        return C.c_char_p if re.fullmatch(r"char \*( \w+)?", " ".join(words)) else _vp
    base = " ".join(words[:-1] if len(words) > 1 else words)       # (the last word of several is the parameter's name)
    if base not in _BY_VALUE:
        raise SlamError("%s: no ctypes rule for %r" % (decl, " ".join(text.split())))
    return _BY_VALUE[base]


def header_signatures(path=HEADER_PATH, text=None):
    """{name: ([argtypes], restype)} of every function include/slam_hip.h declares (or ``text``, a header's contents),
    by the type rule of :func:`_ctype`.  Comments and preprocessor lines are skipped; a statement with a parameter list
    that does not read as ``type name(params)`` raises."""
    if text is None:
        with open(path) as f:
            text = f.read()
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$|\bextern\s+\"C\"\s*\{", " ", text, flags=re.M)
    sigs = {}
    for stmt in text.split(";"):
        if "(" not in stmt:
            continue
        m = re.fullmatch(r"\s*([\w\s*]+?)\s*\b(\w+)\s*\(([^()]*)\)\s*", stmt)
        if m is None:
            raise SlamError("cannot read the declaration %r" % " ".join(stmt.split()))
        res, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        sigs[name] = ([_ctype(name, p) for p in params], _ctype(name, res))
    return sigs


_SIGS = header_signatures()
_SIGS_REFINE = header_signatures(REFINE_HEADER_PATH)
_SIGS_TRACK = header_signatures(TRACK_HEADER_PATH)
NODE_OK, NODE_REF_RAISES, NODE_LM_CAP, NODE_OBS_CAP = 0, 1, 2, 3
LOC_OK, LOC_NONFINITE, LOC_BAD_ROUTE = 0, 1, 2
EKF_MAX_LM = 32
# classes of slam_grid_scan_score (SLAM_RAY_*)
RAY_EMPTY, RAY_HIT, RAY_BLOCKED, RAY_FREE, RAY_UNKNOWN, RAY_OUT, RAY_BAD = range(7)
RAY_CLASSES = 7
# columns of slam_grid_view_gain's counts (SLAM_VIEW_*)
VIEW_UNKNOWN, VIEW_FREE, VIEW_OCCUPIED, VIEW_OPEN = range(4)
VIEW_COUNTS = 4
REFINE_OK, REFINE_BAD_POSE, REFINE_NO_MAP = 0, 1, 2            # status_out of slam_grid_refine (SLAM_REFINE_*)
REFINE_NORMAL_LEN = 9              # normal_out: Hxx, Hxy, Hxt, Hyy, Hyt, Htt, gx, gy, gt
# flag bits of slam_track's info_out (SLAM_TRACK_*) and the row lengths of its state, info and trace
TRACK_MATCHED, TRACK_REFINED, TRACK_INTEGRATED, TRACK_LOST = 1, 2, 4, 8
TRACK_STATE_LEN, TRACK_INFO_LEN, TRACK_TRACE_LEN = 8, 4, 13
MCL_DEAD = 2 ** 31 - 1             # SLAM_MCL_DEAD: a dead particle's accumulated cost
TRAVEL_STRAIGHT, TRAVEL_DIAGONAL, TRAVEL_TRIPS = 10, 14, 1      # SLAM_TRAVEL_*: the two move costs and the trip-bound status
RAY_NAMES = ("empty", "hit", "blocked", "free", "unknown", "out", "bad")


def header_symbols(path=HEADER_PATH):
    """Names of every function include/slam_hip.h declares."""
    return sorted(header_signatures(path))


def lib():
    """Load libslamhip.so once.  Raises LibraryMissing if it was never built."""
    global _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise LibraryMissing(
                    "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    "(or `make -C <package>/csrc`). There is no CPU fallback for this path." % LIB_PATH)
            # One HIP runtime per process: PyTorch-ROCm wheels bundle their own
            # libamdhip64.so.7.  If torch is importable it is loaded FIRST, so that this
            # library's libamdhip64.so.7 dependency resolves to the copy torch uses and
            # device pointers / streams can be shared (bench.py, torch.distributed).  Loading
            # them in the other order leaves torch without a usable device.
            if os.environ.get("SLAM_HIP_STANDALONE") != "1":
                try:
                    import torch  # noqa: F401
                except ImportError:
                    pass
            L = C.CDLL(LIB_PATH)
            for sigs in (_SIGS, _SIGS_REFINE, _SIGS_TRACK):
                for name, (args, res) in sigs.items():
                    fn = getattr(L, name)
                    fn.argtypes, fn.restype = args, res
            if L.slam_abi_version() != 1:
                raise SlamError("libslamhip ABI version %d, binding expects 1" % L.slam_abi_version())
            _lib = L
    return _lib


def _raise(code):
    msg = (lib().slam_last_error() or b"").decode("utf-8", "replace")
    if code == ERR_NAN:
        raise ValueError(msg)            # int(nan) in the reference (mapping.py:33)
    if code == ERR_OVERFLOW:
        raise OverflowError(msg)         # int(inf) in the reference (mapping.py:33)
    if code == ERR_NOMEM:
        raise MemoryError(msg)
    raise SlamError("libslamhip error %d: %s" % (code, msg))


def check(code):
    if code != SLAM_OK:
        _raise(code)


def ptr(a):
    """Host pointer of a C-contiguous ndarray, device pointer of a torch tensor, or an
    int passed through; None -> NULL."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError("array must be C-contiguous")
        return a.ctypes.data
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    return int(a)


class Context:
    """Owns a slam_ctx (one HIP stream + device workspace).  Not thread-safe: one per
    host thread, like the reference's single rospy callback thread."""

    def __init__(self, device=0, stream=None):
        h = _vp()
        check(lib().slam_create(int(device), _vp(stream) if stream else None, C.byref(h)))
        self._h = h
        self.device = int(device)
        self.options = {}              # what set_option last set, by name: the options live on the context, not on its users

    @property
    def handle(self):
        if self._h is None:
            raise SlamError("context already destroyed")
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None:
            lib().slam_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        check(lib().slam_synchronize(self.handle))

    def check_status(self):
        check(lib().slam_check_status(self.handle))

    def stream_order(self, stream, direction):
        """Order this context's work against another HIP stream (``stream``: a raw hipStream_t handle, e.g.
        ``torch.cuda.current_stream().cuda_stream``) without a host synchronise - ``slam_stream_order``:
        direction 0 = that stream waits for everything enqueued here so far, 1 = work enqueued here from now on
        waits for what that stream holds now."""
        check(lib().slam_stream_order(self.handle, _vp(stream) if stream else None, int(direction)))

    def set_option(self, name, value):
        check(lib().slam_set_option(self.handle, name.encode(), float(value)))
        self.options[name] = float(value)

    def timing_enable(self, on=True, only=None):
        """``only``: family names (K_NAMES) whose launches carry events; None: every family."""
        code = int(bool(on))
        if on and only is not None:
            code = 2 * sum(1 << K_NAMES.index(k) for k in only)
        check(lib().slam_timing_enable(self.handle, code))

    def timing_read(self):
        """{family: (milliseconds, launches)} since the last read."""
        ms = np.zeros(len(K_NAMES), dtype=np.float64)
        cnt = np.zeros(len(K_NAMES), dtype=np.int64)
        check(lib().slam_timing_read(self.handle, ptr(ms), ptr(cnt)))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(K_NAMES)}


_default = {}
_default_lock = threading.Lock()


def default_context(device=0):
    """Process-wide context used by the drop-in classes when none is given."""
    with _default_lock:
        c = _default.get(device)
        if c is None or c._h is None:
            c = _default[device] = Context(device)
        return c


def trig_tables(angle_min, angle_max, n):
    """cos/sin of the beam angles exactly as the reference forms them
    (icp.py:227-228): numpy.linspace then numpy.cos / numpy.sin."""
    ang = np.linspace(angle_min, angle_max, n)
    return np.ascontiguousarray(np.cos(ang)), np.ascontiguousarray(np.sin(ang))


def beam_tables(angle_min, angle_increment, n):
    """cos/sin of the beam angles as LocalPlanner.laserCallback forms them
    (local_planner.py:64-68): a = angle_min + angle_increment * i, then math.cos / math.sin."""
    a = [angle_min + angle_increment * i for i in range(n)]
    return (np.array([math.cos(v) for v in a], dtype=np.float64), np.array([math.sin(v) for v in a], dtype=np.float64))
