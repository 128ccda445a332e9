"""Every host-only answer of the library as one JSON document on stdout: the size queries and the bounds-audit entries of
the convolution and weight-gradient launches over a sweep of layers and frames that straddles each rule of the launch
plans (ConvPlan, WgradPlan: csrc/conv.hip, csrc/wgrad.hip).  Needs no GPU (the CU count falls back to 256).  Two trees
whose outputs are byte-equal under every environment setting size, launch and audit alike: the oracle of a refactor of
the launch geometry.

    python tools/host_queries.py > OUT.json        (a fresh process per setting: default, MMLF_CONV_NW16=0,
                                                    MMLF_CONV_RS=0 | 1, MMLF_CONV_CUS=240 -- the library reads them once)

Uses only mmlf_amd._lib, so it runs unchanged in older trees.
"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmlf_amd import _lib                    # noqa: E402

# (K, N): tests/test_bounds_audit.py LAYERS, tests/test_wide_cpu.py WIDE_LAYERS, the 280 -> 1 head and the stream nets' data gradient
LAYERS = [(27, 70), (70, 70), (280, 280), (280, 108), (108, 108), (2, 2), (1, 1),
          (8, 296), (296, 296), (384, 384), (512, 512), (512, 108), (112, 512), (280, 1), (70, 27)]
# (B, H, W): pitch 127 | 128 (sixteen waves), 383 | 384 (one window | two segments), tiny frames, a training batch, a full
# frame, and 42 * 1024 32-position chunks from below and from above (the wide weight gradient's split count)
FRAMES = [(2, 9, 125), (2, 9, 126), (1, 2, 381), (1, 2, 382), (1, 1, 1), (3, 3, 5), (64, 96, 96), (1, 512, 512),
          (143, 96, 96), (144, 96, 96)]


def cs_of(c):
    return (c + 7) // 8 * 8


def audit(fn, n, *args):
    e = (ctypes.c_int64 * n)()
    rc = fn(*args, e)
    return list(e) if rc == 0 else ['refused', _lib.last_error()]


def main():
    L = _lib.load()
    res = {}
    for K, N in LAYERS:
        res[f'filter {K}->{N}'] = {name: getattr(L, name)(K, N) for name in (
            'mmlf_packed_filter_floats', 'mmlf_packed_filter_split_bytes', 'mmlf_packed_filter_h2_bytes',
            'mmlf_packed_filter3x3_floats')}
        res[f'filter {K}->{N}']['mmlf_packed_filter_h2_columns'] = L.mmlf_packed_filter_h2_columns(N)
    for B, H, W in FRAMES:
        P = W + L.mmlf_grid_pad_w()
        res[f'frame {B}x{H}x{W}'] = {'mmlf_relu_mask_words': L.mmlf_relu_mask_words(B, H, W),
                                     'mmlf_audit_relu_bwd_slice': audit(L.mmlf_audit_relu_bwd_slice, 4, 72, 2, 72, 0, 70, 72, B, H, W)}
        for K, N in LAYERS:
            r = res[f'{K}->{N} {B}x{H}x{W}'] = {}
            cs_in, cs_out = cs_of(K), cs_of(N)
            r['mmlf_conv2x2_blocks'] = L.mmlf_conv2x2_blocks(K, N, B, H, W)
            r['mmlf_wgrad_workspace_floats'] = L.mmlf_wgrad_workspace_floats(K, N, B, H, W)
            r['mmlf_wgrad3x3_workspace_floats'] = L.mmlf_wgrad3x3_workspace_floats(K, N, B, H, W)
            for shift in (0, P + 1):
                for n_store in (cs_out, N):
                    r[f'mmlf_audit_conv_h2 shift={shift} n_store={n_store}'] = audit(
                        L.mmlf_audit_conv_h2, 9, cs_in, K, N, cs_out, n_store, shift, cs_out, B, H, W)
                r[f'mmlf_audit_wgrad_h2 g_shift={shift}'] = audit(L.mmlf_audit_wgrad_h2, 7, cs_in, K, cs_out, N, shift, B, H, W)
            for n_store in (cs_out, N):
                r[f'mmlf_audit_conv3x3 n_store={n_store}'] = audit(L.mmlf_audit_conv3x3, 5, cs_in, K, N, cs_out, n_store, cs_out, B, H, W)
            r['mmlf_audit_wgrad3x3'] = audit(L.mmlf_audit_wgrad3x3, 5, cs_in, K, cs_out, N, B, H, W)
    json.dump(res, sys.stdout, indent=0, sort_keys=True)
    print()


if __name__ == '__main__':
    main()
