/*
 * mmlf_eval_hip.h -- C ABI of libmmlf_eval_hip.so, the MI355X (gfx950) kernels of the multimodal evaluation
 * (mmlf_amd/multimodal.py).  A library of its own beside libmmlf_hip.so: the training ABI (include/mmlf_hip.h) and the
 * sources its `src=` hash names do not change when an evaluation kernel does.
 *
 * The reference computes these quantities in post-hoc scripts, pixel by pixel in Python; each entry point names the lines
 * it restates (paths relative to the reference repo root).  Where a script is arbitrary (a randomly initialised KMeans, an
 * argpartition over equal values) the definition chosen here is written at the entry point and in DESIGN.md 4.17.
 *
 * Conventions (those of mmlf_hip.h)
 *  - every pointer is a DEVICE pointer on the current HIP device; the library owns no memory, allocates nothing, never
 *    synchronises and launches on the `stream` it is given (a hipStream_t passed as void*).
 *  - return value: 0 = ok, nonzero = error (bad argument or launch failure); the text is available from
 *    mmlf_eval_last_error() on the calling thread.  Arguments are checked before anything is launched.
 *  - images are (B, H, W) row-major, distributions (B, S, H, W): the bin axis is the slow one, so the 64 lanes of a wave
 *    (one pixel each) read consecutive addresses at every bin.
 *  - no float atomics: sums that leave a workgroup go through float64 partials and a fixed-order second stage, so two
 *    runs give the same bits.
 */
#ifndef MMLF_EVAL_HIP_H
#define MMLF_EVAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char *mmlf_eval_last_error(void);
/* Bumped whenever an entry point's arguments change.  mmlf_eval_abi_version() returns the value the library was BUILT
 * with; mmlf_amd/_lib.py load_eval() compares it with this line before making any other call. */
#define MMLF_EVAL_ABI_VERSION 1
int mmlf_eval_abi_version(void);

/* Largest `radius` of mmlf_eval_gt_modes: 49 offsets lie within 4 pixels, and the kernel sorts them in a fixed LDS tile. */
#define MMLF_EVAL_MAX_RADIUS 4
/* doubles the `partials` workspace of mmlf_eval_two_mode_error must hold */
#define MMLF_EVAL_PARTIALS 6144

/* Two ground-truth modes per pixel (validate/cluster.py:25-64).
 *   gt (B, H, W) float32 -> modes (B, H, W, 2) float64, edges (B, H, W) int32.
 * Edge test: sqrt(sobel_y^2 + sobel_x^2) > edge_threshold with scipy.ndimage.sobel's definition (derivative [-1, 0, 1]
 * along the axis first, then smoothing [1, 2, 1] across it, boundary `reflect`), evaluated in float32 and compared in
 * float64.  A non-edge pixel has both modes equal to gt.  An edge pixel takes the values at the offsets with
 * dy^2 + dx^2 <= radius^2 (coordinates clamped to the image, never another image of the batch), sorts them, and splits them
 * into a lower and an upper non-empty group so that the summed squared deviation from the group means (float64) is
 * smallest; equal minima go to the lowest split index.  The modes are the two group means, ascending: the global optimum
 * of the objective the reference's KMeans descends from a random start.  All values equal: both modes are that value.
 * 0 < radius <= MMLF_EVAL_MAX_RADIUS. */
int mmlf_eval_gt_modes(const float *gt, double *modes, int32_t *edges, int B, int H, int W, double radius,
                       double edge_threshold, void *stream);

/* Modes of a per-pixel distribution over S >= 1 disparity bins.  posterior (B, S, H, W) float32.
 * Raw modes (validate/multimodal.py:44-49, 59-64): a mode is a bin 1 <= j <= S-2 strictly greater than both neighbours; the
 * two strongest win, equal heights go to the lower bin.  n_modes (B, H, W) int32 = min(number of modes, 2);
 * mode_disp (B, H, W, 2) float64 = their disparities j / (S-1) * (disp_max - disp_min) + disp_min, ascending.  With one
 * mode both slots hold it; with none both hold the arg-max bin (lowest index on ties); with S == 1 the fraction
 * j / (S-1) is taken as 0.
 * Mode proportion (utils/modecnt.py:23-75): the bins are smoothed as scipy.ndimage.gaussian_filter1d(sigma, axis=0) does
 * (radius int(4 sigma + 0.5), which must be 8: 1.875 <= sigma < 2.125; float64 weights exp(-0.5 k^2 / sigma^2) over their
 * sum; boundary `reflect` of period 2S; accumulated in float64 over k = -8..8 ascending, rounded to float32 once).  Strict
 * interior maxima and minima are taken on the smoothed values; maxima are kept if (float64) > outlier * the largest one.
 * mode_cnt (B, H, W) int32 = (kept maxima > 1).  mode_prop (B, H, W) float32 = the lower of the two kept maxima that are
 * last in (height, bin) order, divided in float64 by the smallest minimum strictly between their bins (any minimum, as
 * modecnt.py:68 reads); 0 with fewer than two kept maxima or no minimum between them; a zero minimum gives IEEE inf.
 * Any of the four outputs may be NULL (it is then not written). */
int mmlf_eval_posterior_modes(const float *posterior, int32_t *n_modes, double *mode_disp, int32_t *mode_cnt,
                              float *mode_prop, int B, int S, int H, int W, double disp_min, double disp_max,
                              double sigma, double outlier, void *stream);

/* Two-mode error sums (validate/multimodal.py:51-94).  mode_disp, gt_modes (B, H, W, 2) float64; n_modes (B, H, W) int32;
 * gt, pred (B, H, W) float32; out double[6]; partials: MMLF_EVAL_PARTIALS doubles of workspace.
 * Counted pixels: inside the frame less `margin` pixels on every side, with gt_modes[.., 0] != gt_modes[.., 1].
 *   out[0] their count
 *   out[1] multimodal MSE sum: mean over the two slots of (mode_disp_k - gt_modes_k)^2; lb = 1: min_k (gt - mode_disp_k)^2
 *   out[2] multimodal BadPix sum: mean over the slots of |.| > 0.07; lb = 1: the min of the two comparisons
 *   out[3] unimodal MSE sum (gt - pred)^2        out[4] unimodal BadPix sum |gt - pred| > 0.07
 *   out[5] count of those pixels with n_modes < 2
 * All arithmetic in float64.  Sums and counts, never averages: a count of 0 is a result, not a division. */
int mmlf_eval_two_mode_error(const double *mode_disp, const int32_t *n_modes, const double *gt_modes, const float *gt,
                             const float *pred, int B, int H, int W, int margin, int lb, double *partials, double *out,
                             void *stream);

#ifdef __cplusplus
}
#endif
#endif
