"""The persistent 2x2 convolution launches under a cap of the compute units: the case lists of tests/test_gpu_conv_walk.py are
what they claim to be.  No GPU: every figure comes from the library's host queries (tools/host_queries.py shows that they need
none), read in one child process per setting of MMLF_CONV_CUS -- the library reads the variable once per process.

conv4tap_x6s_kernel and conv4tap_rs_kernel (csrc/conv.hip) launch `cus` or `2 * cus` workgroups (conv_plan), each of which walks
the tiles t, t + grid, t + 2 grid, ...; the chunk pipeline, the f16 split's operand scale (next_amax -> scale_a), the
accumulators, run_max and the BatchNorm sums cross a tile boundary inside that loop.  On 256 compute units every frame of the
suite's edge lists is one tile per workgroup, so none of that runs where the suite is strict.  MMLF_CONV_CUS = 8 | 9 makes
small frames walk: 8 and 16 workgroups take the kernels' XCD-ordered branch, 9 and 18 the linear one.

Asserted here, for the cases the GPU file runs:
  * with the cap unset every case is one trip -- the premise;
  * under each cap every case takes at least three trips (trips = ceil(tiles / workgroups), tiles of 256 or 512 positions),
    and every kernel family has a case whose last trip is ragged;
  * cap 8 gives workgroup counts divisible by 8, cap 9 none;
  * every kernel family meets both placements, ReLU on and off, whole rows and a channel slice, the stream pairs the three
    variants;
  * in the mixed-magnitude leg every tiled case has a hand-over (tiles t -> t + workgroups of one workgroup: a tiled-kernel
    workgroup owns a residue class of the tiles, whatever the XCD permutation) across which the tile maximum rises by at
    least 2^10, and one across which it falls by as much.

The constants below are the GPU file's as well."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CAPS = (None, 8, 9)
MODES = ('f16x3', 'bf16x6')                   # the persistent arithmetic paths; 'f32' (one workgroup per tile) is the control
# image b is scaled by 2^E_CYCLE[b % 6] (tests/test_gpu_precision.py test_conv_patches_of_very_different_magnitude: small after
# big and big after small); on frames of fewer than four images bands of four grid rows are, by the same cycle
E_CYCLE = (0, -10, -20, -30, 0, -30)
BAND_ROWS = 4
# (B, H, W): 32 tiles of 256 positions | 28 (ragged at 8 workgroups: 3 trips + 4) | pitch 127, 128 (sixteen-wave kernel |
# eight-wave and register-streamed kernels) | pitch 383, 384 (one activation window | two segments) | pitch 132 | pitch 302
FRAMES = [(6, 33, 37), (5, 33, 37), (6, 12, 125), (6, 12, 126), (2, 12, 381), (2, 12, 382), (3, 24, 130), (1, 40, 300)]
TILED_LAYERS = [(280, 280), (70, 70), (27, 70), (280, 108), (108, 108), (8, 32)]
BLOCK_LAYERS = [(72, 296), (296, 296), (72, 512), (512, 72), (8, 289)]            # column blocks: 289 ... 512 channels
THIN_LAYERS = [(280, 1), (280, 2), (70, 2)]
STREAM_PAIRS = [(27, 70), (70, 70)]           # the layers that run under the stream variants 1 and 2
FAMILIES = ('wide', 'sixteen', 'narrow8', 'rs', 'two_segment', 'column_blocks', 'thin')

# (frame, (K, N), pad, variant, relu, sliced), filled in below the transcribed launch plan: the exact-integer leg runs the
# forward launch K -> N with these options and the data gradient of an N -> K layer (the same launch shape) at this placement;
# the mixed-magnitude leg runs both at the other placement, the forward launch with the other ReLU and slice setting.
CASES = []
# the exact-f32 launches are not persistent: one frame, as a control of the test itself
F32_CASES = [((5, 33, 37), (280, 280), 1, 0, True, False), ((5, 33, 37), (70, 70), 0, 2, False, True)]
# the epilogue's BatchNorm sums (f16 split, pad-0 forward): (frame, (K, N))
BN_CASES = [((6, 12, 125), (70, 70)), ((6, 12, 126), (70, 70)), ((5, 33, 37), (280, 280)), ((6, 12, 125), (296, 296))]
# the thin kernels: (frame, (K, N), pad, variant)
THIN_CASES = [((6, 12, 125), (280, 1), 1, 0), ((1, 40, 300), (280, 2), 0, 2), ((2, 12, 382), (70, 2), 1, 1),
              ((3, 24, 130), (280, 2), 0, 0)]
NET_FRAME = (6, 33, 37)                       # the 70-channel model_no_batchnorm net

QUERY = r'''
import json, sys
sys.path.insert(0, %r)
from mmlf_amd import _lib
L = _lib.load()
frames, layers = json.loads(sys.argv[1])
res = {'cus': L.mmlf_conv_cus(), 'pad_w': L.mmlf_grid_pad_w(), 'pad_h': L.mmlf_grid_pad_h()}
for B, H, W in frames:
    res['words %%d %%d %%d' %% (B, H, W)] = L.mmlf_relu_mask_words(B, H, W)
    for K, N in layers:
        res['blocks %%d %%d %%d %%d %%d' %% (K, N, B, H, W)] = L.mmlf_conv2x2_blocks(K, N, B, H, W)
        res['wgrad_ws %%d %%d %%d %%d %%d' %% (K, N, B, H, W)] = L.mmlf_wgrad_workspace_floats(K, N, B, H, W)
for K in sorted({k for k, n in layers}):
    res['thin_ws %%d' %% K] = L.mmlf_conv2x2_wgrad_thin_workspace_floats(K)
print(json.dumps(res))
''' % ROOT


def cap_env(cap):
    """the environment of a child under this cap: MMLF_CONV_MODE removed, MMLF_CONV_CUS set or removed"""
    env = dict(os.environ)
    env.pop('MMLF_CONV_MODE', None)
    env.pop('MMLF_CONV_CUS', None)
    if cap is not None:
        env['MMLF_CONV_CUS'] = str(cap)
    return env


@pytest.fixture(scope='module')
def queries():
    """{cap: the host queries' answers}, one child process per cap"""
    arg = json.dumps([FRAMES, TILED_LAYERS + BLOCK_LAYERS + THIN_LAYERS])
    out = {}
    for cap in CAPS:
        res = subprocess.run([sys.executable, '-c', QUERY, arg], env=cap_env(cap), capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr[-3000:]
        out[cap] = json.loads(res.stdout.strip().splitlines()[-1])
    return out


# ---------------------------------------------------------------------------------------------- the launch plan, transcribed
def pitch(frame):
    return frame[2] + 2


def positions(frame):
    """grid positions B x (H + 2) x (W + 2)"""
    return frame[0] * (frame[1] + 2) * (frame[2] + 2)


def tiles256(frame):
    """256-position tiles of the padded grid (padded to whole 512-position tiles: csrc/common.h make_grid)"""
    return (positions(frame) + 511) // 512 * 2


def packed_columns(N):
    """columns of ONE launch (csrc/conv.hip x6_np, wide_np / col_blocks)"""
    if N > 288:
        return (320 if N <= 320 else 384 if N <= 384 else 512) // 2
    return 32 if N <= 32 else 80 if N <= 80 else (N + 15) // 16 * 16 if N <= 128 else 288


def plan(mode, K, N, frame, cus):
    """csrc/conv.hip conv_plan for the two split paths: (kernel family, tile positions, tiles, workgroups).  The f16 figures
    are held to mmlf_conv2x2_blocks below; the bf16 split has no sixteen-wave and no register-streamed kernel."""
    npb, nchunk, P = packed_columns(N), (K + 7) // 8, pitch(frame)
    f16 = mode == 'f16x3'
    sixteen = f16 and npb == 80 and P + 513 <= 640
    rs = f16 and npb == 80 and nchunk in (4, 9) and not sixteen
    tile = 512 if sixteen else 256
    ntiles = tiles256(frame) * 256 // tile
    narrow = npb // 16 <= 6 and not sixteen and not rs
    grid = 2 * cus if narrow else cus
    fam = 'sixteen' if sixteen else 'rs' if rs else 'narrow8' if narrow else 'wide'
    return fam, tile, ntiles, min(grid, ntiles)


def families(mode, K, N, frame):
    """every family a case counts for: its kernel, the two-segment activation window of the tiled kernels (pitch + tile + 1
    positions do not fit the 640 slots), the column blocks"""
    fam, tile, _, _ = plan(mode, K, N, frame, 256)
    out = {fam}
    if fam != 'rs' and pitch(frame) + tile + 1 > 640:
        out.add('two_segment')
    if N > 288:
        out.add('column_blocks')
    return out


def trips(ntiles, blocks):
    return -(-ntiles // blocks)


def row_exponents(frame, off, h):
    """exponent of every grid row of the mixed-magnitude leg, None where the operand (extent of h rows at grid offset `off`)
    is zero: by image from four images on, else by bands of four grid rows"""
    B, H, W = frame
    out = []
    for b in range(B):
        for r in range(H + 2):
            inside = off <= r < off + h
            out.append((E_CYCLE[b % 6] if B >= 4 else E_CYCLE[r // BAND_ROWS % 6]) if inside else None)
    return out


def tile_exponents(frame, tile, ntiles, off, h):
    """the exponent of a tile's maximum: over the grid rows its positions and their taps read, [t tile, (t + 1) tile + P + 1]"""
    P = pitch(frame)
    rows = row_exponents(frame, off, h)
    out = []
    for t in range(ntiles):
        r0, r1 = t * tile // P, ((t + 1) * tile + P + 1) // P
        es = [e for e in rows[r0:r1 + 1] if e is not None]
        out.append(max(es) if es else None)
    return out


def _cases():
    """every layer on every frame that takes three trips under both caps in both split modes (the sixteen-wave kernel's
    512-position tiles and the narrow kernels' 2 x cus workgroups leave the 33 x 37 frames at two: those layers skip them), the
    options rotated over layers and frames so that every family meets every one (asserted below)"""
    out = []
    for j, (K, N) in enumerate(TILED_LAYERS + BLOCK_LAYERS):
        for i, frame in enumerate(FRAMES):
            if any(trips(*plan(mode, K, N, frame, cap)[2:]) < 3 for mode in MODES for cap in (8, 9)):
                continue
            variant = (i + j) % 3 if (K, N) in STREAM_PAIRS else 0
            out.append((frame, (K, N), (i + j) % 2, variant, (j + i // 2) % 2 == 0, (i + j // 2) % 2 == 1))
    return out


CASES += _cases()


# ---------------------------------------------------------------------------------------------- the tests
def test_the_case_lists_name_known_frames_and_layers():
    for frame, layer, pad, variant, relu, sliced in CASES + F32_CASES:
        assert frame in FRAMES and layer in TILED_LAYERS + BLOCK_LAYERS
        assert variant == 0 or layer in STREAM_PAIRS
    assert {c[1] for c in CASES} == set(TILED_LAYERS + BLOCK_LAYERS)
    assert {c[0] for c in CASES} == set(FRAMES)
    assert {c[1] for c in THIN_CASES} == set(THIN_LAYERS) and all(c[0] in FRAMES for c in THIN_CASES)
    assert len(CASES) == 11 * 8 - 4 * 2                    # four narrow layers skip the two 33 x 37 frames
    assert {c[1] for c in BN_CASES} == {(70, 70), (280, 280), (296, 296)}
    assert all((frame, layer) in {(c[0], c[1]) for c in CASES} for frame, layer in BN_CASES)


def test_the_transcribed_plan_is_the_librarys(queries):
    """grid pads, tile counts and, for the f16 split, the workgroup count of every (layer, frame) under every cap"""
    for cap in CAPS:
        q = queries[cap]
        assert (q['pad_w'], q['pad_h']) == (2, 2)
        assert q['cus'] == (cap or 256), 'the host fallback is 256 compute units'
        for frame in FRAMES:
            assert q['words %d %d %d' % frame] == tiles256(frame) * 4096
            for K, N in TILED_LAYERS + BLOCK_LAYERS:
                assert q['blocks %d %d %d %d %d' % (K, N, *frame)] == plan('f16x3', K, N, frame, q['cus'])[3], (cap, K, N, frame)
    # the families are where the issue puts them
    assert plan('f16x3', 70, 70, (6, 12, 125), 256)[0] == 'sixteen' and plan('f16x3', 70, 70, (6, 12, 126), 256)[0] == 'rs'
    assert plan('f16x3', 27, 70, (3, 24, 130), 256)[0] == 'rs' and plan('bf16x6', 70, 70, (6, 12, 126), 256)[0] == 'narrow8'
    assert plan('f16x3', 8, 32, (6, 12, 126), 256)[0] == 'narrow8' and plan('f16x3', 280, 108, (2, 12, 381), 256)[0] == 'wide'
    assert 'two_segment' in families('f16x3', 280, 280, (2, 12, 382)) and 'two_segment' not in families('f16x3', 280, 280, (2, 12, 381))


def test_uncapped_every_case_is_one_trip(queries):
    """the premise: on 256 compute units no launch of these cases walks"""
    cus = queries[None]['cus']
    for frame, (K, N), *_ in CASES:
        for mode in MODES:
            _, _, ntiles, blocks = plan(mode, K, N, frame, cus)
            assert blocks == ntiles and trips(ntiles, blocks) == 1, (mode, K, N, frame)
    for frame, (K, N), *_ in THIN_CASES:
        # thin_rowdot_kernel: 4 cus workgroups of four waves, 64 positions a wave and trip, over NQ + P + 1 positions;
        # thin_wgrad_kernel: 16 cus waves, the same positions
        assert positions(frame) + pitch(frame) + 2 <= 64 * 16 * cus


@pytest.mark.parametrize('cap', [8, 9])
def test_capped_every_case_walks_three_trips_and_every_family_has_a_ragged_last_trip(queries, cap):
    cus = queries[cap]['cus']
    assert cus == cap
    ragged, seen = set(), set()
    for frame, (K, N), *_ in CASES:
        for mode in MODES:
            fam, _, ntiles, blocks = plan(mode, K, N, frame, cus)
            assert blocks in (cus, 2 * cus) and (blocks % 8 == 0) == (cap == 8), (mode, K, N, frame, blocks)
            assert trips(ntiles, blocks) >= 3, (mode, K, N, frame, ntiles, blocks)
            fams = families(mode, K, N, frame)
            seen |= fams
            if ntiles % blocks:
                ragged |= fams
    # the thin kernels have no tiles: their waves stride over 64-position pieces, at these frames two trips with a ragged second
    for frame, (K, N), *_ in THIN_CASES:
        pieces, waves = -(-(positions(frame) + pitch(frame) + 2) // 64), 16 * cus
        assert queries[cap]['thin_ws %d' % K] == waves * 4 * (K + 1) * 2          # (the weight gradient's waves)
        assert trips(pieces, waves) >= 2, (frame, pieces, waves)
        seen.add('thin')
        if pieces % waves:
            ragged.add('thin')
    assert seen == set(FAMILIES), set(FAMILIES) - seen
    assert ragged == set(FAMILIES), set(FAMILIES) - ragged


def test_the_workspace_queries_follow_the_cap(queries):
    """what the GPU file sizes its workspaces by: the thin weight gradient's follows the cap (one slab per wave); the split
    weight gradients' is positive under every cap"""
    for cap in CAPS:
        q = queries[cap]
        for frame, (K, N), *_ in THIN_CASES:
            assert q['thin_ws %d' % K] == 16 * q['cus'] * 4 * (K + 1) * 2
            assert q['wgrad_ws %d %d %d %d %d' % (K, N, *frame)] > 0
    assert queries[8]['thin_ws 280'] < queries[9]['thin_ws 280'] < queries[None]['thin_ws 280']


def test_every_family_meets_every_option():
    """both placements, ReLU on and off, whole rows and a channel slice in the exact-integer leg (the mixed-magnitude leg
    runs the complement, so it meets both as well); the three variants on the stream pairs"""
    seen = {f: {'pad': set(), 'relu': set(), 'sliced': set()} for f in FAMILIES if f != 'thin'}
    variants = {p: set() for p in STREAM_PAIRS}
    for frame, (K, N), pad, variant, relu, sliced in CASES:
        for mode in MODES:
            for f in families(mode, K, N, frame):
                seen[f]['pad'].add(pad)
                seen[f]['relu'].add(relu)
                seen[f]['sliced'].add(sliced)
        if (K, N) in variants:
            variants[(K, N)].add(variant)
    for f, opts in seen.items():
        for name, vals in opts.items():
            assert len(vals) == 2, (f, name, vals)
    assert all(v == {0, 1, 2} for v in variants.values()), variants
    assert {c[2] for c in THIN_CASES} == {0, 1} and {c[3] for c in THIN_CASES} == {0, 1, 2}


@pytest.mark.parametrize('cap', [8, 9])
def test_mixed_magnitude_hand_overs_rise_and_fall_by_2_to_the_10(queries, cap):
    """per tiled case, mode and operand placement of the mixed-magnitude leg: a workgroup's consecutive tiles t, t + workgroups
    whose maxima differ by at least 2^10 upwards, and a pair that differs as much downwards.  (The register-streamed kernel
    takes a group's scale when it reaches the group: no hand-over.)"""
    cus = queries[cap]['cus']
    for frame, (K, N), pad, *_ in CASES:
        B, H, W = frame
        for mode in MODES:
            fam, tile, ntiles, blocks = plan(mode, K, N, frame, cus)
            if fam == 'rs':
                continue
            # the forward launch reads x (pad 1: H rows at grid offset 1, pad 0: H + 1 rows at 0); the data gradient of the
            # other placement reads a gradient that lies where that forward's output does
            for off, h in ((1, H), (0, H + 1)):
                e = tile_exponents(frame, tile, ntiles, off, h)
                steps = [e[t + blocks] - e[t] for t in range(ntiles - blocks) if e[t] is not None and e[t + blocks] is not None]
                assert steps and max(steps) >= 10 and min(steps) <= -10, (mode, K, N, frame, cap, steps)
