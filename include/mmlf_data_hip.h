/*
 * mmlf_data_hip.h -- C ABI of libmmlf_data_hip.so, the MI355X (gfx950) kernels of the composable training patch chain
 * (mmlf_amd/patches.py PatchPipeline(chain=...), mmlf_amd/transforms.py).  A fourth library beside
 * libmmlf_hip.so, libmmlf_eval_hip.so and libmmlf_ese_hip.so: their ABIs (include/mmlf_hip.h, mmlf_eval_hip.h,
 * mmlf_ese_hip.h) and the sources their hashes name do not change when one of these kernels does.
 *
 * The reference composes a training sample from the transforms of mmlf/data/hci4d.py:416-1090 on the CPU, over the whole
 * frame.  Here the scenes stay in device memory and a batch is one gather of the ps x ps output pixels (mmlf_data_gather)
 * plus one pass for the two transforms that need the finished patch (mmlf_data_finish: Contrast, Noise).  The fixed CLI
 * chain keeps its own entry points in libmmlf_hip.so (mmlf_patch_gather, mmlf_patch_contrast); the per-pixel arithmetic
 * here is theirs, operation for operation.
 *
 * Conventions (those of mmlf_hip.h)
 *  - every pointer is a DEVICE pointer on the current HIP device; the library owns no memory, allocates nothing, never
 *    synchronises and launches on the `stream` it is given (a hipStream_t passed as void*).
 *  - return value: 0 = ok, nonzero = error (bad argument or launch failure); the text is available from
 *    mmlf_data_last_error() on the calling thread.  Arguments are checked before anything is launched.
 */
#ifndef MMLF_DATA_HIP_H
#define MMLF_DATA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char *mmlf_data_last_error(void);
/* Bumped whenever an entry point's arguments change.  mmlf_data_abi_version() returns the value the library was BUILT
 * with; mmlf_amd/_lib.py load_data() compares it with this line before making any other call. */
#define MMLF_DATA_ABI_VERSION 1
int mmlf_data_abi_version(void);

/* flags of iparam[b][6] */
#define MMLF_DATA_SHEAR 1      /* two-tap shear (Shift): taps tab_s, weights tab_w; gt and mpi[:, 4] minus disp */
#define MMLF_DATA_COLOR 2      /* RedistColor: mat[b] */
#define MMLF_DATA_BRIGHT 4     /* Brightness: times fparam[b][2] */
#define MMLF_DATA_ROLL 8       /* one-tap shear (IntegerShift): tap tab_s[..][0] alone; gt and mpi[:, 4] minus disp */
#define MMLF_DATA_GT_MUL 16    /* Zoom: gt and mpi[:, 4] times fparam[b][0] */
#define MMLF_DATA_GT_DIV 32    /* DownSampling: gt and mpi[:, 4] divided by fparam[b][0] */

/* The gather: scale (through index tables), circular shear over the scaled frame, crop, rotation, colour matrix and
 * brightness, per output pixel.
 *   stacks (S,4,V,3,Hf,Wf), center (S,3,Hf,Wf), gt (S,Hf,Wf), mpi (S,P,5,Hf,Wf) or NULL with P=0, mask (S,Hf,Wf) int32.
 *   Per sample b (all drawn and computed on the host):
 *   iparam[b] = {scene, hs, ws, y0, x0, rot, flags, 0}: the extents of the SCALED frame, the crop's origin in it
 *               (0 <= y0, y0 + ps <= hs; likewise x), the number of Rotate90 steps and the MMLF_DATA_* flags.
 *   fparam[b] = {gt scale, disp, brightness, 0}.
 *   ymap[b][0..hs) and xmap[b][0..ws) (int32, rows of map_h and map_w entries): the cached frame's row / column behind
 *               every row / column of the scaled frame -- o * f for DownSampling, scipy.ndimage.zoom(order=0)'s source
 *               index for Zoom, the identity without a scale.  Every entry lies in [0, Hf) / [0, Wf), or is -1: the
 *               row / column scipy fills with its constant (mmlf_amd/transforms.py zoom_map), read as zero in every
 *               plane.  The shear's taps wrap modulo hs / ws and go through the same tables.
 *   tab_s/tab_w[b][view] = (shift0, shift1) / (1 - alpha, alpha) as mmlf_shift_views takes them; a roll of |s| >= the
 *               extent is the identity.  mat[b] = 3x3 RedistColor matrix (double).
 *   rot_src[rot][stack][view] = source stack*V + view after `rot` Rotate90 steps.
 * Outputs: o_stacks (4,B,V,3,ps,ps), o_center (B,3,ps,ps), o_gt (B,ps,ps), o_mpi (B,P,5,ps,ps), o_mask (B,ps,ps) (not
 * rotated, hci4d.py:1056); mean_sum[b] (float64, zeroed by the caller, may be NULL) accumulates the sum of the
 * horizontal stack as written, for Contrast (one atomic add per output row: float32 values summed in double). */
int mmlf_data_gather(const float *stacks, const float *center, const float *gt, const float *mpi, const int32_t *mask,
                     int S, int V, int P, int Hf, int Wf, const int32_t *iparam, const float *fparam,
                     const int32_t *ymap, int map_h, const int32_t *xmap, int map_w, const int32_t *tab_s,
                     const float *tab_w, const double *mat, const int32_t *rot_src, float *o_stacks, float *o_center,
                     float *o_gt, float *o_mpi, int32_t *o_mask, double *mean_sum, int B, int ps, void *stream);

/* Contrast and Noise in one pass, in place on o_stacks (4,B,V,3,ps,ps) and o_center (B,3,ps,ps); either may be absent.
 *   Contrast (alpha != NULL; hci4d.py:740-751): x*alpha[b][0] + mean_b*alpha[b][1] with alpha[b] = {float(a),
 *   float(1 - a)} and mean_b = mean_sum[b] / (V*3*ps*ps).
 *   Noise (noise != 0; hci4d.py:811-816): x = float(double(x) + double(stdev) * z), z ~ N(0, 1) independent per element.
 *   z comes from Philox4x32-10 keyed by `seed`, with the counter (element index / 4, call), and the Box-Muller transform
 *   of its four words (two pairs): the same seed, call and shapes give the same bits.  It is not NumPy's stream.
 * Contrast comes first, as the slot order has it. */
int mmlf_data_finish(float *o_stacks, float *o_center, const double *mean_sum, const float *alpha, int noise,
                     float stdev, int64_t seed, int64_t call, int B, int V, int ps, void *stream);

#ifdef __cplusplus
}
#endif
#endif
