"""ctypes loader for libansfm.so (the HIP/gfx950 engine behind include/ansfm.h).

The library is built in-tree (archnemesis_dist_amd/lib/libansfm.so) by `build()` /
`__graft_entry__.build()`.  There is NO CPU fallback: if the library is missing or no HIP device
is usable, this module raises -- product code never routes through the CPU oracle.
"""
import ctypes as C
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libansfm.so")
CSRC = os.path.join(_HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(_HERE), "include")

ANSFM_OK = 0
ERR_NAMES = {1: "ANSFM_ERR_INVALID", 2: "ANSFM_ERR_HIP", 3: "ANSFM_ERR_NOTABLE", 4: "ANSFM_ERR_UNSORTED",
             5: "ANSFM_ERR_UNSUPPORTED"}

_BY_VALUE = {"int": C.c_int, "unsigned int": C.c_uint, "double": C.c_double, "int64_t": C.c_int64}
_RETURNS = {"int": C.c_int, "void": None, "const char *": C.c_char_p}


def prototypes(header):
    """{name: (restype, argtypes)} of every `ret ansfm_name(args);` in the text of include/ansfm.h, in its order.  A pointer or
    array parameter is a c_void_p (a plain `const char *`: c_char_p); int, unsigned int, double and int64_t go by value.
    Anything else raises, with the prototype named: the header has grown a type this table does not know."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header, flags=re.S)        # comments
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)                  # preprocessor lines
    norm = lambda d: " ".join(d.replace("*", " * ").split())              # one blank between tokens, `*` a token
    out = {}
    for ret, name, args in re.findall(r"([^;{}()]*?)\b(ansfm_\w+)\s*\(([^()]*)\)\s*;", text):
        proto = f"{norm(ret)} {name}({norm(args)})"
        if norm(ret) not in _RETURNS:
            raise AnsfmError(f"include/ansfm.h: unknown return type in `{proto}`")
        argtypes = []
        for decl in ([] if norm(args) in ("", "void") else [norm(d) for d in args.split(",")]):
            if "*" in decl or "[" in decl:
                argtypes.append(C.c_char_p if re.fullmatch(r"const char \* \w+", decl) else C.c_void_p)
                continue
            by_value = " ".join(w for w in decl.split()[:-1] if w != "const")     # without the parameter's name
            if by_value not in _BY_VALUE:
                raise AnsfmError(f"include/ansfm.h: unknown type of parameter `{decl}` in `{proto}`")
            argtypes.append(_BY_VALUE[by_value])
        out[name] = (_RETURNS[norm(ret)], argtypes)
    return out


class AnsfmError(RuntimeError):
    pass


# the one statement of the C-ABI is include/ansfm.h: the ctypes prototypes and the list of symbols are read from it
PROTOTYPES = prototypes(open(os.path.join(INCLUDE, "ansfm.h")).read())
EXPORTS = list(PROTOTYPES)

_lib = None


def hipcc_path():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


def build(force=False, verbose=False):
    """Compile the HIP sources for gfx950 into lib/libansfm.so (cross-compiles without a GPU)."""
    srcs = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))
    deps = srcs + [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(INCLUDE, "ansfm.h")]
    if not force and os.path.exists(LIB_PATH):
        newest = max(os.path.getmtime(d) for d in deps)
        if os.path.getmtime(LIB_PATH) >= newest:
            return LIB_PATH
    os.makedirs(os.path.dirname(LIB_PATH), exist_ok=True)
    # one object per translation unit, compiled side by side, then one link
    from concurrent.futures import ThreadPoolExecutor
    flags = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-fvisibility=hidden"]
    objs = [os.path.join(os.path.dirname(LIB_PATH), os.path.splitext(os.path.basename(src))[0] + ".o") for src in srcs]

    def compile_one(pair):
        src, obj = pair
        cmd = [hipcc_path()] + flags + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)

    with ThreadPoolExecutor(max_workers=min(len(srcs), 8)) as pool:
        list(pool.map(compile_one, zip(srcs, objs)))
    cmd = [hipcc_path(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objs
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB_PATH


def _preload_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64.so; libansfm.so is linked against the
    one under /opt/rocm.  Whichever is loaded first must serve both, or the second initialisation fails (seen as
    torch.cuda.is_available() == False after an engine was created).  If torch is installed and not yet imported, its
    copy is loaded first (by path, no `import torch`), so libansfm.so's DT_NEEDED entry resolves to it."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return                                         # torch's runtime is already the process's runtime
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    path = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(path):
        try:
            C.CDLL(path, mode=C.RTLD_GLOBAL)
        except OSError:
            pass                                       # fall back on the system runtime; torch must then be imported first


def load():
    """dlopen libansfm.so and declare prototypes.  Raises AnsfmError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AnsfmError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    _preload_torch_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)                        # AttributeError: the library lacks a symbol the header declares
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def read_ktable_header(path):
    """Spectroscopy_0.read_ktahead (:2492) through the native reader (no GPU needed):
    nwave, wave, fwhm, npress, ntemp, ng, gasID, isoID, g_ord, del_g, presslevels, templevels."""
    import numpy as np
    lib = load()
    dims = (C.c_int64 * 4)(); ids = (C.c_int32 * 2)(); hdr = (C.c_double * 3)()
    if lib.ansfm_ktable_file_header(os.fsencode(path), dims, ids, hdr, None, None, None, None, None) != ANSFM_OK:
        raise ValueError("not a readable .kta table: %s" % path)
    nwave, ng, npress, ntemp = (int(d) for d in dims)
    wave = np.empty(nwave); g_ord = np.empty(ng, np.float32); del_g = np.empty(ng, np.float32)
    press = np.empty(npress, np.float32); temp = np.empty(ntemp, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.ansfm_ktable_file_header(os.fsencode(path), dims, ids, hdr, p(wave), p(g_ord), p(del_g), p(press), p(temp))
    return nwave, wave, float(hdr[2]), npress, ntemp, ng, int(ids[0]), int(ids[1]), g_ord, del_g, press, temp


def read_lbltable_header(path):
    """Spectroscopy_0.read_ltahead (:2451) through the native reader (no GPU needed):
    nwave, vmin, delv, npress, ntemp, gasID, isoID, presslevels, templevels  (+ the wavenumber grid as a 10th item)."""
    import numpy as np
    lib = load()
    dims = (C.c_int64 * 3)(); ids = (C.c_int32 * 2)(); hdr = (C.c_double * 2)()
    if lib.ansfm_lbltable_file_header(os.fsencode(path), dims, ids, hdr, None, None, None) != ANSFM_OK:
        raise ValueError("not a readable .lta table: %s" % path)
    nwave, npress, ntemp = (int(d) for d in dims)
    # NT < 0: one grid of -NT temperatures per pressure level (the reference's reader returns them as (npress, -NT), :2480-2483)
    tshape = (npress, -ntemp) if ntemp < 0 else (ntemp,)
    wave = np.empty(nwave); press = np.empty(npress, np.float32); temp = np.empty(tshape, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.ansfm_lbltable_file_header(os.fsencode(path), dims, ids, hdr, p(wave), p(press), p(temp))
    return nwave, float(hdr[0]), float(hdr[1]), npress, ntemp, int(ids[0]), int(ids[1]), press, temp, wave
