"""Loader of the in-tree C-ABI library (libauroralz.so).  Fails loudly: there is no CPU fallback."""
import ctypes as C
import os

from . import _abi as A

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libauroralz.so")
_lib = None
# Set when this process first makes a call that initialises HIP (alz_create, alz_device_count ...).  From then on nothing here starts a compiler: on the GPU pool a process that has
# touched the GPU must not fork + exec (the lazy builders -- synth.py here, the checker library of the tests -- ask this and tell the caller to run `__graft_entry__.build()` instead).
GPU_TOUCHED = False


def refuse_build_after_gpu(what):
    if GPU_TOUCHED:
        raise RuntimeError("%s is missing or older than its source, and this process has already initialised the GPU: build first "
                           "(python -c 'import __graft_entry__ as g; g.build()'), a compiler is not started from here" % what)


class AlzError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("auroralz error %d: %s" % (code, msg))
        self.code = code


def _preload_hip_runtime():
    """One HIP runtime per process: if torch is installed its bundled libamdhip64.so (SONAME libamdhip64.so.7)
    is loaded first, so both torch and libauroralz.so bind to the same runtime instance."""
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec and spec.origin:
            p = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
            if os.path.exists(p):
                C.CDLL(p, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
                          "auroralib.compression_amd has no CPU fallback." % SO_PATH)
    _preload_hip_runtime()
    lib = C.CDLL(SO_PATH)
    for name, types in A.PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.argtypes = types
        fn.restype = A.RESTYPES.get(name, C.c_int)
    if lib.alz_abi_version() != A.ABI_VERSION:
        raise ImportError("libauroralz.so ABI %d != python mirror %d" % (lib.alz_abi_version(), A.ABI_VERSION))
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise AlzError(rc, load().alz_last_error().decode("utf-8", "replace"))
