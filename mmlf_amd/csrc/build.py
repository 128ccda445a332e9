"""Build libmmlf_hip.so (gfx950) in-tree with hipcc.  `python -m mmlf_amd.csrc.build`."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCES = ['conv.hip', 'wgrad.hip', 'elementwise.hip']
LIB = os.path.join(HERE, 'libmmlf_hip.so')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
# -ffp-contract=off: elementwise kernels restate float32 expressions of the reference op by op
# (mul, mul, add); fused multiply-adds appear only where written (fmaf / MFMA).
FLAGS = ['-O3', '--offload-arch=gfx950', '-fPIC', '-std=c++17', '-Wall', '-Wno-unused-function', '-ffp-contract=off']


def stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = SOURCES + ['common.h', 'conv_device.h', 'wgrad_map.h', 'row_walk.h', 'build.py', os.path.join('..', '..', 'include', 'mmlf_hip.h')]
    return any(os.path.getmtime(os.path.join(HERE, d)) > t for d in deps)


def source_revision():
    """short git hash of the tree the library is built from ('+' if the kernel sources differ from it), for mmlf_build_info()"""
    root = os.path.dirname(os.path.dirname(HERE))
    try:
        rev = subprocess.check_output(['git', '-C', root, 'rev-parse', '--short=12', 'HEAD'], stderr=subprocess.DEVNULL).decode().strip()
        dirty = subprocess.call(['git', '-C', root, 'diff', '--quiet', 'HEAD', '--', 'mmlf_amd/csrc', 'include'],
                                stderr=subprocess.DEVNULL) != 0
        return rev + ('+' if dirty else '')
    except (OSError, subprocess.CalledProcessError):
        return 'unknown'          # (no git on the GPU box's snapshot: the library that travels there was built here)


HASHED = SOURCES + ['common.h', 'conv_device.h', 'wgrad_map.h', 'row_walk.h', os.path.join('..', '..', 'include', 'mmlf_hip.h')]


def source_hash():
    """content hash of everything the kernels are compiled from: mmlf_build_info()'s `src=` field.  Unlike `git=` (the HEAD
    the library happened to be built at: build.stale() looks at file times, not at HEAD) it names the kernel sources
    themselves -- bench.py compares it between the library it times and the one the committed PMC passes were collected on."""
    import hashlib
    h = hashlib.sha1()
    for d in HASHED:
        with open(os.path.join(HERE, d), 'rb') as f:
            h.update(f.read())
    return h.hexdigest()[:12]


def build(force=False, verbose=True, extra_flags=(), lib=None):
    """extra_flags / lib: another build of the same sources somewhere else (tests/test_gpu_bounds.py: -DMMLF_BOUNDS_DEBUG)"""
    if lib is None and not extra_flags and not force and not stale():
        return LIB
    lib = lib or LIB
    tag = '' if lib == LIB else '.' + os.path.basename(lib).replace('.so', '')
    flags = [*FLAGS, f'-DMMLF_GIT_HASH="{source_revision()}"', f'-DMMLF_SRC_HASH="{source_hash()}"', *extra_flags]
    objs, jobs = [], []
    for src in SOURCES:                 # the translation units are independent: compiled side by side
        obj = os.path.join(os.path.dirname(lib), src.replace('.hip', tag + '.o'))
        cmd = [HIPCC, *flags, '-c', os.path.join(HERE, src), '-o', obj]
        if verbose:
            print(' '.join(cmd), flush=True)
        jobs.append((cmd, subprocess.Popen(cmd)))
        objs.append(obj)
    failed = [cmd for cmd, job in jobs if job.wait() != 0]
    if failed:
        raise subprocess.CalledProcessError(1, failed[0])
    cmd = [HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC', *objs, '-o', lib]
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.check_call(cmd)
    return lib


# The multimodal evaluation (include/mmlf_eval_hip.h) is a library of its own: none of its files is in SOURCES or HASHED, so
# neither libmmlf_hip.so nor its `src=` hash changes when an evaluation kernel does.
EVAL_SOURCES = ['evaluate.hip']
EVAL_LIB = os.path.join(HERE, 'libmmlf_eval_hip.so')
EVAL_HEADER = os.path.join(HERE, '..', '..', 'include', 'mmlf_eval_hip.h')


def eval_stale():
    if not os.path.exists(EVAL_LIB):
        return True
    t = os.path.getmtime(EVAL_LIB)
    deps = [os.path.join(HERE, s) for s in EVAL_SOURCES] + [os.path.join(HERE, 'build.py'), EVAL_HEADER]
    return any(os.path.getmtime(d) > t for d in deps)


def build_eval(force=False, verbose=True):
    """libmmlf_eval_hip.so, with the FLAGS of the training library (-ffp-contract=off: its float64 arithmetic is written
    operation by operation)"""
    if not force and not eval_stale():
        return EVAL_LIB
    cmd = [HIPCC, *FLAGS, '-shared', *[os.path.join(HERE, s) for s in EVAL_SOURCES], '-o', EVAL_LIB]
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.check_call(cmd)
    return EVAL_LIB


# The Ensamble's backward kernels (include/mmlf_ese_hip.h): a third library on the same terms -- none of its files is in
# SOURCES, HASHED or EVAL_SOURCES.
ESE_SOURCES = ['ensamble_grad.hip']
ESE_LIB = os.path.join(HERE, 'libmmlf_ese_hip.so')
ESE_HEADER = os.path.join(HERE, '..', '..', 'include', 'mmlf_ese_hip.h')


def ese_stale():
    if not os.path.exists(ESE_LIB):
        return True
    t = os.path.getmtime(ESE_LIB)
    deps = [os.path.join(HERE, s) for s in ESE_SOURCES] + [os.path.join(HERE, 'build.py'), ESE_HEADER]
    return any(os.path.getmtime(d) > t for d in deps)


def build_ese(force=False, verbose=True):
    """libmmlf_ese_hip.so, with the FLAGS of the training library (-ffp-contract=off: its float32 sums are written
    operation by operation)"""
    if not force and not ese_stale():
        return ESE_LIB
    cmd = [HIPCC, *FLAGS, '-shared', *[os.path.join(HERE, s) for s in ESE_SOURCES], '-o', ESE_LIB]
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.check_call(cmd)
    return ESE_LIB


# The composable patch chain (include/mmlf_data_hip.h): a fourth library on the same terms -- none of its files is in
# SOURCES, HASHED, EVAL_SOURCES or ESE_SOURCES.
DATA_SOURCES = ['patch_chain.hip']
DATA_LIB = os.path.join(HERE, 'libmmlf_data_hip.so')
DATA_HEADER = os.path.join(HERE, '..', '..', 'include', 'mmlf_data_hip.h')


def data_stale():
    if not os.path.exists(DATA_LIB):
        return True
    t = os.path.getmtime(DATA_LIB)
    deps = [os.path.join(HERE, s) for s in DATA_SOURCES] + [os.path.join(HERE, 'build.py'), DATA_HEADER]
    return any(os.path.getmtime(d) > t for d in deps)


def build_data(force=False, verbose=True):
    """libmmlf_data_hip.so, with the FLAGS of the training library (-ffp-contract=off: the gather restates
    mmlf_patch_gather's float32 arithmetic operation by operation)"""
    if not force and not data_stale():
        return DATA_LIB
    cmd = [HIPCC, *FLAGS, '-shared', *[os.path.join(HERE, s) for s in DATA_SOURCES], '-o', DATA_LIB]
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.check_call(cmd)
    return DATA_LIB


# The scene builder (include/mmlf_scene_hip.h): a fifth library on the same terms -- none of its files is in SOURCES, HASHED,
# EVAL_SOURCES, ESE_SOURCES or DATA_SOURCES.
SCENE_SOURCES = ['scene.hip']
SCENE_LIB = os.path.join(HERE, 'libmmlf_scene_hip.so')
SCENE_HEADER = os.path.join(HERE, '..', '..', 'include', 'mmlf_scene_hip.h')


def scene_stale():
    if not os.path.exists(SCENE_LIB):
        return True
    t = os.path.getmtime(SCENE_LIB)
    deps = [os.path.join(HERE, s) for s in SCENE_SOURCES] + [os.path.join(HERE, 'build.py'), SCENE_HEADER]
    return any(os.path.getmtime(d) > t for d in deps)


def build_scene(force=False, verbose=True):
    """libmmlf_scene_hip.so, with the FLAGS of the training library (-ffp-contract=off: the texture mask's float32 sum and
    its one division are written operation by operation)"""
    if not force and not scene_stale():
        return SCENE_LIB
    cmd = [HIPCC, *FLAGS, '-shared', *[os.path.join(HERE, s) for s in SCENE_SOURCES], '-o', SCENE_LIB]
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.check_call(cmd)
    return SCENE_LIB


if __name__ == '__main__':
    if '--source-hash' in sys.argv:
        print(source_hash())
    elif '--source-revision' in sys.argv:
        print(source_revision())
    else:
        build(force='--force' in sys.argv)
        build_eval(force='--force' in sys.argv)
        build_ese(force='--force' in sys.argv)
        build_data(force='--force' in sys.argv)
        build_scene(force='--force' in sys.argv)
