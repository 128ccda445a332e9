/*
 * mmlf_ese_hip.h -- C ABI of libmmlf_ese_hip.so, the MI355X (gfx950) kernels of the Ensamble's backward pass
 * (mmlf_amd/ensamble.py).  A third library beside libmmlf_hip.so and libmmlf_eval_hip.so: the training ABI
 * (include/mmlf_hip.h), the evaluation ABI (include/mmlf_eval_hip.h) and the sources their hashes name do not change when
 * one of these kernels does.
 *
 * The reference's Ensamble (mmlf/model/ensamble.py:40-118) is torch code that autograd differentiates; the two entry points
 * are the adjoints of the two kernels the forward pass launches around the members (mmlf_ensamble_reduce, mmlf_shift_pack).
 *
 * Conventions (those of mmlf_hip.h)
 *  - every pointer is a DEVICE pointer on the current HIP device; the library owns no memory, allocates nothing, never
 *    synchronises and launches on the `stream` it is given (a hipStream_t passed as void*).
 *  - return value: 0 = ok, nonzero = error (bad argument or launch failure); the text is available from
 *    mmlf_ese_last_error() on the calling thread.  Arguments are checked before anything is launched.
 *  - no atomics: every sum is taken by one thread in a fixed order, so two runs give the same bits and the result does not
 *    depend on the launch geometry.
 */
#ifndef MMLF_ESE_HIP_H
#define MMLF_ESE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char *mmlf_ese_last_error(void);
/* Bumped whenever an entry point's arguments change.  mmlf_ese_abi_version() returns the value the library was BUILT
 * with; mmlf_amd/_lib.py load_ese() compares it with this line before making any other call. */
#define MMLF_ESE_ABI_VERSION 1
int mmlf_ese_abi_version(void);

/* (member, view) table entries one mmlf_ese_unshift_sum launch holds in LDS: n * views may not exceed it (the caller
 * splits the members; the output is accumulated into, so two launches over halves give one launch's sum) */
#define MMLF_ESE_MAX_TAB 2048

/* Backward of mmlf_ensamble_reduce (ensamble.py:78-101).
 *   means, logvars (S, B, H, W); grid[S]; g_mean, g_logvar (B, H, W); g_posterior (B, S, H, W); all float32.
 *   g_means, g_logvars (S, B, H, W): EVERY element is written.  Each of the three incoming gradients may be NULL (= zero).
 * With b_j = expf(logvar_j), a_kj = |grid_k - m_j| / b_j and L_kj = expf(-a_kj) / (2 b_j), per pixel
 *   g_m_j  = (1/S) sum_k g_posterior_k L_kj sign(grid_k - m_j) / b_j          (sign(0) = 0: the gradient of torch's abs)
 *   g_lv_j = (1/S) sum_k g_posterior_k L_kj (a_kj - 1)
 * summed over k ascending in float32; g_mean and g_logvar are then added at the arg-min member of logvar, found as the
 * forward kernel finds it (strict <: the lowest index wins a tie). */
int mmlf_ese_reduce_bwd(const float *means, const float *logvars, const float *grid, const float *g_mean,
                        const float *g_logvar, const float *g_posterior, float *g_means, float *g_logvars, int S, int B,
                        int H, int W, void *stream);

/* Adjoint of mmlf_shift_pack for one view stack, summed over the members.
 *   g: the gradient of n members in the trunk's grid layout -- member s, position (y, x), channel c at
 *      ((s (H + 2) + y + 1) (W + 2) + x + 1) cs + c; only channels [0, 3 views) of interior positions are read.
 *   kind: 0 = horizontal stack, 1 = vertical, 2 = increasing diagonal (the opposite sign along H), 3 = decreasing diagonal.
 *   tab_s (n, views, 2) int32, tab_w (n, views, 2) float32: the shift table of THESE members (mmlf_shift_pack's).
 *   out (views, 3, H, W) float32: ACCUMULATED into.
 * The forward is a gather through roll_src; the adjoint is the same gather with every integer shift negated (a shift of
 * |s| >= the extent is the identity in both).  The taps of one member are combined as the forward combines them
 * (w0 a + w1 b; the diagonal kinds along W first, then along H), the members are added in member order.
 * cs % 4 == 0, 3 views <= cs, n views <= MMLF_ESE_MAX_TAB. */
int mmlf_ese_unshift_sum(const float *g, int cs, int kind, const int32_t *tab_s, const float *tab_w, int n, int views, int H,
                         int W, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
