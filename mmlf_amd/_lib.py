"""ctypes binding of libmmlf_hip.so (the C ABI declared in include/mmlf_hip.h).

The product path has no CPU fallback: if the library is missing or a call fails, a
RuntimeError is raised (with the text from ``mmlf_last_error()``).
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# MMLF_HIP_LIB selects another build of the same ABI (kernel A/B experiments); never a fallback
LIB_PATH = os.environ.get('MMLF_HIP_LIB') or os.path.join(_HERE, 'csrc', 'libmmlf_hip.so')

_HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'mmlf_hip.h')
_CTYPES = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'long long': ctypes.c_longlong,
           'double': ctypes.c_double, 'float': ctypes.c_float}


def signatures_from_header(text):
    """{name: (restype, [argtypes])} of every prototype in a C header written like include/mmlf_hip.h: comments,
    preprocessor lines, `typedef struct {...} name;` and `enum {...};` are skipped, everything else must be
    `ret name(params);`.  Any pointer or array declarator is a c_void_p (a `const char *` result a c_char_p), a scalar one
    of _CTYPES; whatever is not recognised raises with the prototype's text -- a guessed argument type would shift every
    argument behind it."""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    text = re.sub(r'^[ \t]*#(?:[^\n]*\\\n)*[^\n]*', ' ', text, flags=re.M)
    text = re.sub(r'\btypedef\s+struct\b[^{;]*\{[^{}]*\}[^;]*;', ' ', text)
    text = re.sub(r'\benum\b[^{;]*\{[^{}]*\}\s*;', ' ', text)
    text = re.sub(r'\bextern\s+"C"\s*\{', ' ', text).replace('}', ' ')     # (its closing brace stands alone)

    def scalar(words, proto):
        key = ' '.join(w for w in words.split() if w != 'const')
        if key not in _CTYPES:
            raise ValueError(f'C header: unknown type `{words.strip()}` in `{proto}`')
        return _CTYPES[key]

    sigs = {}
    for stmt in text.split(';'):
        proto = ' '.join(stmt.split())
        if not proto:
            continue
        m = re.fullmatch(r'([\w\s\*]+?)\b(\w+) ?\(([^()]*)\)', proto)
        if m is None or m.group(2) in sigs:
            raise ValueError(f'C header: cannot parse `{proto}`')
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        if '*' in ret:
            if ret.split() != ['const', 'char', '*']:
                raise ValueError(f'C header: unknown return type `{ret.strip()}` in `{proto}`')
            res = ctypes.c_char_p
        else:
            res = scalar(ret, proto)
        args = []
        for param in ([] if params == 'void' else params.split(',')):
            d = re.fullmatch(r'\s*([\w\s\*]*?[\w\*])\s*\b(\w+)\s*((?:\[\w*\])?)\s*', param)
            if d is None or not re.search(r'\w', d.group(1)):
                raise ValueError(f'C header: cannot parse parameter `{param.strip()}` of `{proto}`')
            args.append(ctypes.c_void_p if '*' in d.group(1) or d.group(3) else scalar(d.group(1), proto))
        sigs[name] = (res, args)
    return sigs


def _header_text():
    with open(_HEADER) as f:
        return f.read()


# name -> (restype, argtypes) of every entry point: include/mmlf_hip.h is the one place that declares them (the compiler
# holds the definitions in csrc/ to the same file)
SIGNATURES = signatures_from_header(_header_text())


def _header_abi_version():
    """MMLF_ABI_VERSION as include/mmlf_hip.h defines it: ONE place holds the number (the library returns the same macro)"""
    m = re.search(r'^#define\s+MMLF_ABI_VERSION\s+(\d+)', _header_text(), re.M)
    if m is None:
        raise RuntimeError(f'{_HEADER}: no MMLF_ABI_VERSION')
    return int(m.group(1))


ABI_VERSION = _header_abi_version()     # bumped whenever an entry point's arguments change
_lib = None
BUILD_INFO = None


def validate(lib, path, environ=None):
    """Refuse a library this package must not call: another ABI version (its entry points would be called with shifted
    arguments) or a build that computes WRONG results by construction -- the timing ablations of older trees
    (`mmlf_build_is_ablation()`; tools/README.md "Removed"), unless MMLF_ALLOW_ABLATION=1 says the user wants exactly that (kernel A/B runs).
    `lib` is anything with the three entry points (the tests pass a stub).  Returns the build string."""
    environ = os.environ if environ is None else environ
    got = lib.mmlf_abi_version() if hasattr(lib, 'mmlf_abi_version') else None
    if got != ABI_VERSION:
        raise RuntimeError(f'{path} implements ABI version {got}, this package needs {ABI_VERSION}: rebuild it '
                           'with `python -m mmlf_amd.csrc.build --force`')
    if not hasattr(lib, 'mmlf_build_info') or not hasattr(lib, 'mmlf_build_is_ablation'):
        raise RuntimeError(f'{path} does not say what it was built with (no mmlf_build_info): rebuild it')
    info = lib.mmlf_build_info()
    info = info.decode() if isinstance(info, bytes) else str(info)
    if lib.mmlf_build_is_ablation() and environ.get('MMLF_ALLOW_ABLATION') != '1':
        raise RuntimeError(f'{path} is a timing-ablation build that computes WRONG results ({info}); it is refused unless '
                           'MMLF_ALLOW_ABLATION=1 is set (unset MMLF_HIP_LIB to use the product library)')
    return info


def load():
    """Load the shared library once; raise if it is absent (no fallback)."""
    global _lib, BUILD_INFO
    if _lib is None:
        # torch FIRST: it ships a HIP runtime of its own (torch/lib/libamdhip64.so) and this library is linked against the
        # system's (/opt/rocm/lib).  Loaded in the other order the process holds two runtimes and the first launch fails with
        # "no ROCm-capable device is detected" (seen when `python __graft_entry__.py smoke` loaded the library in build(), before
        # anything had imported torch); with torch's runtime already mapped the loader resolves this library's dependency to it:
        # this module imports torch at its top.
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f'{LIB_PATH} not found: build it with `python -m mmlf_amd.csrc.build` '
                '(the HIP path has no CPU fallback)')
        lib = ctypes.CDLL(LIB_PATH)
        for name in ('mmlf_abi_version', 'mmlf_build_info', 'mmlf_build_is_ablation'):
            if hasattr(lib, name):
                getattr(lib, name).restype, getattr(lib, name).argtypes = SIGNATURES[name]
        BUILD_INFO = validate(lib, LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def build_info():
    """the loaded library's mmlf_build_info() string (bench.py prints it in config.build)"""
    load()
    return BUILD_INFO


def last_error():
    return load().mmlf_last_error().decode()


def call(name, *args):
    """Invoke an int-returning entry point; nonzero status -> RuntimeError."""
    rc = getattr(load(), name)(*args)
    if rc != 0:
        raise RuntimeError(f'{name} failed: {last_error()}')


# ---- libmmlf_eval_hip.so: the multimodal evaluation kernels (include/mmlf_eval_hip.h), an ABI of their own ----
EVAL_LIB_PATH = os.path.join(_HERE, 'csrc', 'libmmlf_eval_hip.so')
_EVAL_HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'mmlf_eval_hip.h')


def _eval_header_text():
    with open(_EVAL_HEADER) as f:
        return f.read()


EVAL_SIGNATURES = signatures_from_header(_eval_header_text())
EVAL_ABI_VERSION = int(re.search(r'^#define\s+MMLF_EVAL_ABI_VERSION\s+(\d+)', _eval_header_text(), re.M).group(1))
_eval_lib = None


def load_eval():
    """Load libmmlf_eval_hip.so once; raise if it is absent or of another ABI version (no fallback).  torch is imported at
    this module's top, ahead of the library, for the reason load() gives."""
    global _eval_lib
    if _eval_lib is None:
        if not os.path.exists(EVAL_LIB_PATH):
            raise RuntimeError(f'{EVAL_LIB_PATH} not found: build it with `python -m mmlf_amd.csrc.build` '
                               '(the multimodal evaluation has no fallback on CUDA tensors)')
        lib = ctypes.CDLL(EVAL_LIB_PATH)
        got = lib.mmlf_eval_abi_version() if hasattr(lib, 'mmlf_eval_abi_version') else None
        if got != EVAL_ABI_VERSION:
            raise RuntimeError(f'{EVAL_LIB_PATH} implements ABI version {got}, this package needs {EVAL_ABI_VERSION}: '
                               'rebuild it with `python -m mmlf_amd.csrc.build --force`')
        for name, (res, args) in EVAL_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _eval_lib = lib
    return _eval_lib


def call_eval(name, *args):
    """Invoke an int-returning entry point of the evaluation library; nonzero status -> RuntimeError."""
    lib = load_eval()
    if getattr(lib, name)(*args) != 0:
        raise RuntimeError(f'{name} failed: {lib.mmlf_eval_last_error().decode()}')


# ---- libmmlf_ese_hip.so: the Ensamble's backward kernels (include/mmlf_ese_hip.h), an ABI of their own ----
ESE_LIB_PATH = os.path.join(_HERE, 'csrc', 'libmmlf_ese_hip.so')
_ESE_HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'mmlf_ese_hip.h')


def _ese_header_text():
    with open(_ESE_HEADER) as f:
        return f.read()


ESE_SIGNATURES = signatures_from_header(_ese_header_text())
ESE_ABI_VERSION = int(re.search(r'^#define\s+MMLF_ESE_ABI_VERSION\s+(\d+)', _ese_header_text(), re.M).group(1))
ESE_MAX_TAB = int(re.search(r'^#define\s+MMLF_ESE_MAX_TAB\s+(\d+)', _ese_header_text(), re.M).group(1))
_ese_lib = None


def load_ese():
    """Load libmmlf_ese_hip.so once; raise if it is absent or of another ABI version (no fallback).  torch is imported at
    this module's top, ahead of the library, for the reason load() gives."""
    global _ese_lib
    if _ese_lib is None:
        if not os.path.exists(ESE_LIB_PATH):
            raise RuntimeError(f'{ESE_LIB_PATH} not found: build it with `python -m mmlf_amd.csrc.build` '
                               '(the Ensamble\'s backward has no fallback on CUDA tensors)')
        lib = ctypes.CDLL(ESE_LIB_PATH)
        got = lib.mmlf_ese_abi_version() if hasattr(lib, 'mmlf_ese_abi_version') else None
        if got != ESE_ABI_VERSION:
            raise RuntimeError(f'{ESE_LIB_PATH} implements ABI version {got}, this package needs {ESE_ABI_VERSION}: '
                               'rebuild it with `python -m mmlf_amd.csrc.build --force`')
        for name, (res, args) in ESE_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _ese_lib = lib
    return _ese_lib


def call_ese(name, *args):
    """Invoke an int-returning entry point of the Ensamble-backward library; nonzero status -> RuntimeError."""
    lib = load_ese()
    if getattr(lib, name)(*args) != 0:
        raise RuntimeError(f'{name} failed: {lib.mmlf_ese_last_error().decode()}')


# ---- libmmlf_data_hip.so: the composable patch chain's kernels (include/mmlf_data_hip.h), an ABI of their own ----
DATA_LIB_PATH = os.path.join(_HERE, 'csrc', 'libmmlf_data_hip.so')
_DATA_HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'mmlf_data_hip.h')


def _data_header_text():
    with open(_DATA_HEADER) as f:
        return f.read()


DATA_SIGNATURES = signatures_from_header(_data_header_text())
DATA_ABI_VERSION = int(re.search(r'^#define\s+MMLF_DATA_ABI_VERSION\s+(\d+)', _data_header_text(), re.M).group(1))
DATA_FLAGS = {name: int(value) for name, value in
              re.findall(r'^#define\s+MMLF_DATA_(SHEAR|COLOR|BRIGHT|ROLL|GT_MUL|GT_DIV)\s+(\d+)', _data_header_text(), re.M)}
_data_lib = None


def load_data():
    """Load libmmlf_data_hip.so once; raise if it is absent or of another ABI version (no fallback).  torch is imported at
    this module's top, ahead of the library, for the reason load() gives."""
    global _data_lib
    if _data_lib is None:
        if not os.path.exists(DATA_LIB_PATH):
            raise RuntimeError(f'{DATA_LIB_PATH} not found: build it with `python -m mmlf_amd.csrc.build` '
                               '(PatchPipeline(chain=...) has no fallback)')
        lib = ctypes.CDLL(DATA_LIB_PATH)
        got = lib.mmlf_data_abi_version() if hasattr(lib, 'mmlf_data_abi_version') else None
        if got != DATA_ABI_VERSION:
            raise RuntimeError(f'{DATA_LIB_PATH} implements ABI version {got}, this package needs {DATA_ABI_VERSION}: '
                               'rebuild it with `python -m mmlf_amd.csrc.build --force`')
        for name, (res, args) in DATA_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _data_lib = lib
    return _data_lib


def call_data(name, *args):
    """Invoke an int-returning entry point of the patch-chain library; nonzero status -> RuntimeError."""
    lib = load_data()
    if getattr(lib, name)(*args) != 0:
        raise RuntimeError(f'{name} failed: {lib.mmlf_data_last_error().decode()}')


# ---- libmmlf_scene_hip.so: the scene builder's kernels (include/mmlf_scene_hip.h), an ABI of their own ----
SCENE_LIB_PATH = os.path.join(_HERE, 'csrc', 'libmmlf_scene_hip.so')
_SCENE_HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'mmlf_scene_hip.h')


def _scene_header_text():
    with open(_SCENE_HEADER) as f:
        return f.read()


SCENE_SIGNATURES = signatures_from_header(_scene_header_text())
SCENE_ABI_VERSION = int(re.search(r'^#define\s+MMLF_SCENE_ABI_VERSION\s+(\d+)', _scene_header_text(), re.M).group(1))
SCENE_MAX_WSIZE = int(re.search(r'^#define\s+MMLF_SCENE_MAX_WSIZE\s+(\d+)', _scene_header_text(), re.M).group(1))
_scene_lib = None


def load_scene_lib():
    """Load libmmlf_scene_hip.so once; raise if it is absent or of another ABI version (no fallback).  torch is imported
    at this module's top, ahead of the library, for the reason load() gives."""
    global _scene_lib
    if _scene_lib is None:
        if not os.path.exists(SCENE_LIB_PATH):
            raise RuntimeError(f'{SCENE_LIB_PATH} not found: build it with `python -m mmlf_amd.csrc.build` '
                               '(mmlf_amd.scenes has no fallback on CUDA tensors)')
        lib = ctypes.CDLL(SCENE_LIB_PATH)
        got = lib.mmlf_scene_abi_version() if hasattr(lib, 'mmlf_scene_abi_version') else None
        if got != SCENE_ABI_VERSION:
            raise RuntimeError(f'{SCENE_LIB_PATH} implements ABI version {got}, this package needs {SCENE_ABI_VERSION}: '
                               'rebuild it with `python -m mmlf_amd.csrc.build --force`')
        for name, (res, args) in SCENE_SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _scene_lib = lib
    return _scene_lib


def call_scene(name, *args):
    """Invoke an int-returning entry point of the scene library; nonzero status -> RuntimeError."""
    lib = load_scene_lib()
    if getattr(lib, name)(*args) != 0:
        raise RuntimeError(f'{name} failed: {lib.mmlf_scene_last_error().decode()}')


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def check(t, name, device, dtype=torch.float32, shape=None, numel=None, min_numel=None, contiguous=True):
    """Hold a tensor that a caller supplied to what the kernel behind `ptr(t)` takes on trust: it lives on `device`, has
    `dtype` (None: any, the caller converts) and the exact `shape`, exactly `numel` or at least `min_numel` elements, and is
    contiguous.  Called where such a tensor enters the native path, ahead of the first launch: a raw pointer of another
    device or a shorter tensor is a GPU memory fault, another dtype or stride order a quietly wrong result.  Reads the
    tensor's metadata only (any device, `meta` included); never the pointer, never the library."""
    ok = (t is not None and t.device == device and dtype in (None, t.dtype) and (shape is None or tuple(t.shape) == tuple(shape))
          and (numel is None or t.numel() == numel) and (min_numel is None or t.numel() >= min_numel)
          and (not contiguous or t.is_contiguous()))
    if not ok:
        found = 'None' if t is None else f'{t.dtype} {tuple(t.shape)} on {t.device}, contiguous={t.is_contiguous()}'
        need = ', '.join(f'{k}={v}' for k, v in (('dtype', dtype), ('shape', shape if shape is None else tuple(shape)),
                                                 ('numel', numel), ('min_numel', min_numel),
                                                 ('contiguous', contiguous or None)) if v is not None)
        raise ValueError(f'{name}: found {found}; required on {device}: {need}')


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream
