/*
 * Geometric self-ensemble ("x8" test-time augmentation) for the KDLAE HIP library: the two device steps either
 * side of the forwards.  Same library, same conventions as kdlae.h (status codes, the thread-local
 * kdlae_last_error text, the caller's-stream contract of its opening paragraph); the ABI version stays 1.
 *
 * The rule.  Mode m in 0..7 is
 *
 *     T_m(x) = flipud^(m % 2)( rot90ccw^(m / 2)(x) )        on the last two axes,
 *
 * numpy's np.rot90(x, k = m / 2) followed by np.flipud when m is odd: the `data_augmentation` modes the three
 * networks are trained under.  Modes 0, 1, 4, 5 keep [H, W]; modes 2, 3, 6, 7 give [W, H].  For a set of modes
 * M, given as an 8-bit mask (bit m = mode m), a model f and an image x with its rate map,
 *
 *     y   = ( (((0 + U_m0) + U_m1) + ...) ) / float(|M|)      m0 < m1 < ...: ascending modes
 *     U_m = T_m^-1( f(T_m(x), T_m(rate)) )
 *
 * in fp32, every add and the one divide rounded on their own.  The rate map is transformed with the image; an
 * output at twice the size (sr) is merged by the same rule at [2H, 2W].  M = {0} gives f(x)'s bits (a -0 comes
 * out as +0: it is 0 + U).  y is a different function of the image from f(x): the mean of f over the views, not
 * an approximation of f(x) that carries an error bound.
 *
 * Slot layout.  Both entries see the views as one dense block [N][C][H'][W'] per set bit of the mask, packed
 * back to back in ascending mode order: slot s (the s-th set bit) starts at float s * N * C * H * W, whatever the
 * shapes of the slots before it, and holds |M| * N * C * H * W floats in all.
 *
 * Both entries: no handle, no workspace, no host wait, no allocation; one kernel launch on `stream`, so the call
 * can be captured into a graph.  Refused with KDLAE_EINVAL_SHAPE and a last-error text before anything is
 * launched: a null pointer, N, C, H or W <= 0, mode_mask == 0 or mode_mask > 255.  H and W are otherwise
 * arbitrary.  src and dst must not overlap.  16-byte loads and stores are used when src and dst sit on 16 bytes
 * and W % 4 == 0, 4-byte ones otherwise; the bits of the result do not depend on which.
 */
#ifndef KDLAE_ENSEMBLE_H_
#define KDLAE_ENSEMBLE_H_

#include "kdlae.h"

#ifdef __cplusplus
extern "C" {
#endif

/* src [N][C][H][W] -> dst: slot s = T_m(src) for the s-th set mode m, [N][C][H][W] or [N][C][W][H]. */
int kdlae_ens_gather(const float* src, float* dst, int N, int C, int H, int W, int mode_mask, void* stream);

/* src: per-view outputs in the slot layout for an [N][C][H][W] result (slot s = the s-th set mode's output, in
 * that view's orientation) -> dst [N][C][H][W] = the rule's y: per pixel the inverse-transformed values added in
 * ascending mode order to 0, then divided by the number of modes. */
int kdlae_ens_merge(const float* src, float* dst, int N, int C, int H, int W, int mode_mask, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KDLAE_ENSEMBLE_H_ */
