/*
 * mmlf_scene_hip.h -- C ABI of libmmlf_scene_hip.so, the MI355X (gfx950) kernels that build a cached training scene from
 * decoded view images (mmlf_amd/scenes.py).  A fifth library beside libmmlf_hip.so, libmmlf_eval_hip.so,
 * libmmlf_ese_hip.so and libmmlf_data_hip.so: their ABIs (include/mmlf_hip.h, mmlf_eval_hip.h, mmlf_ese_hip.h,
 * mmlf_data_hip.h) and the sources their hashes name do not change when one of these kernels does.
 *
 * The reference builds a scene on the CPU in HCI4D.load_scene (mmlf/data/hci4d.py:124-254): it picks four view stacks out
 * of the camera grid, converts them to float CHW, cuts the centre view and multiplies the scene's mask by
 * create_mask_texture(center, 23, 0.02) (hci4d.py:38-69, 241), whose `unfold` materialises 3 * wsize^2 * H * W floats.
 * Here the stacks are one pass over the decoded images (mmlf_scene_pack_views) and the texture mask is one kernel that
 * walks each pixel's window out of LDS (mmlf_scene_texture).
 *
 * Conventions (those of mmlf_hip.h)
 *  - every pointer is a DEVICE pointer on the current HIP device; the library owns no memory, allocates nothing, never
 *    synchronises and launches on the `stream` it is given (a hipStream_t passed as void*).
 *  - return value: 0 = ok, nonzero = error (bad argument or launch failure); the text is available from
 *    mmlf_scene_last_error() on the calling thread.  Arguments are checked before anything is launched.
 */
#ifndef MMLF_SCENE_HIP_H
#define MMLF_SCENE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char *mmlf_scene_last_error(void);
/* Bumped whenever an entry point's arguments change.  mmlf_scene_abi_version() returns the value the library was BUILT
 * with; mmlf_amd/_lib.py load_scene_lib() compares it with this line before making any other call. */
#define MMLF_SCENE_ABI_VERSION 1
int mmlf_scene_abi_version(void);

/* largest window of mmlf_scene_texture (odd sizes 1..63) */
#define MMLF_SCENE_MAX_WSIZE 63

/* The texture mask of hci4d.create_mask_texture, optionally times a scene mask.
 *   center (B,3,H,W) float32; wsize odd, 1 <= wsize <= MMLF_SCENE_MAX_WSIZE (an even size is refused: the reference's
 *   `view` fails on it); mask_in (B,H,W) int32 or NULL; mask_out (B,H,W) int32 or NULL; mae_out (B,H,W) float32 or NULL;
 *   at least one of the two outputs.
 *   mae = (sum over the 3 * wsize^2 window values of |x - c_channel|) / (3 * wsize^2), the window zero-padded outside the
 *   frame (unfold's padding: a border pixel compares against zeros).  The sum is taken in float32, channel after
 *   channel, window row after window row, left to right; the quotient is ONE IEEE float32 division of that sum by
 *   float(3 * wsize^2).  mae_out holds exactly that float32.
 *   mask_out = (mae >= (float)threshold) -- a NaN gives 0 --, zero in the wsize / 2 margin, times mask_in where given.
 *   A frame with H or W <= 2 * (wsize / 2) is all margin: mask_out is zero everywhere, mae_out still defined.
 *   3 * B * H * W must stay below 2^31. */
int mmlf_scene_texture(const float *center, int wsize, double threshold, const int32_t *mask_in, int32_t *mask_out,
                       float *mae_out, int B, int H, int W, void *stream);

/* Decoded images (HWC, file order) to the four CHW float stacks and the centre view, in one pass.
 *   Exactly one of grid_u8 (N,H,W,3) uint8 and grid_f32 (N,H,W,3) float32 is given.  lut (256) float32: a uint8 value v
 *   becomes lut[v] (the kernel does no arithmetic on it; NULL is refused with grid_u8); a float grid is copied.
 *   sel (4 * V) int32: sel[s * V + k] is the grid image behind view k of stack s.  It is a device array like every other
 *   pointer here, so the CALLER holds every entry to [0, N) on the host before the call (mmlf_amd/scenes.py pack_views
 *   does); the kernel writes nothing for a slot whose entry lies outside that range and never reads through it.
 *   center_slot in [0, 4 * V): the sel slot whose image is also written to center (3,H,W).
 *   stacks (4,V,3,H,W) float32.  N * H * W * 3 and 4 * V * 3 * H * W must stay below 2^31. */
int mmlf_scene_pack_views(const uint8_t *grid_u8, const float *grid_f32, const float *lut, const int32_t *sel,
                          int center_slot, int N, int V, int H, int W, float *stacks, float *center, void *stream);

#ifdef __cplusplus
}
#endif
#endif
