/*
 * libvstyler -- Wan2.2-Animate's motion encoder (diffsynth/models/wan_video_animate_adapter.py:321-612,
 * Generator.get_motion): everything between the convolutions of its StyleGAN2-style encoder.  The
 * convolutions and the linears themselves are vs_vae_conv and vs_gemm.
 *
 * An eighth header of the same library and the same conventions as vstyler.h: bf16 raw 16-bit values,
 * launches on `stream`, no allocation, 0 (VS_OK) or a VS_E_* code, every shape / stride / alignment /
 * overlap violation rejected before anything is launched.  vs_abi_version() is unchanged (the entries are
 * additions) and they read no option.
 *
 * Activations are channels-last frames [n][H][W][ld], frames `ns` elements apart, as vs_vae_conv reads
 * them with t_in = 1.  r() is round-to-nearest-even to bf16; all arithmetic is fp32.
 *
 * ACT(x, b) = r( r( lrelu( r(x + b) ) ) * s2 ),  lrelu(a) = a >= 0 ? a : a * 0.2f,  s2 = (float)2**0.5:
 * the reference's fused_leaky_relu, F.leaky_relu(input + bias, 0.2) * 2**0.5, on bf16 tensors (three
 * roundings).  One device function shared by the first three entries.
 */
#ifndef VSTYLER_MOTION_H
#define VSTYLER_MOTION_H

#include "vstyler.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The stem, ConvLayer(3, c0, 1): face frames -> ACT(conv1x1) in channels-last form.
 *
 * x: x_u8 != 0: uint8 [n][h][w][3], px = r( r((float)u8 * (float)(2/255)) + (-1) ) (preprocess_image on a
 * bf16 pipeline); x_u8 == 0: bf16 planar [3][n][h][w] (the reference's face_pixel_values of one sample),
 * px the value itself.  Both contiguous.  wt: the prepared bf16 weight [c0][3], bias bf16 [c0].
 *     c[co] = r( fma(px_2, w[co][2], fma(px_1, w[co][1], px_0 * w[co][0])) ),  y[.., co] = ACT(c[co], bias[co]).
 * y: [n][h][w][ldy], frames y_ns apart; columns >= c0 are not written.
 *
 * c0 % 8 == 0, c0 <= 512; ldy >= c0, ldy % 8 == 0; y_ns >= (h w - 1) ldy + c0, y_ns % 8 == 0; wt, bias and y
 * 16-byte aligned (x 2-byte aligned when bf16); y overlaps none of x, wt, bias.
 */
int vs_motion_stem(const void* x, int x_u8, const void* wt, const void* bias, void* y, long long y_ns,
                   long long ldy, int n, int h, int w, int c0, void* stream);

/*
 * The reference's Blur (upfirdn2d with k = [1,3,3,1] (x) [1,3,3,1] / 64, pad (p0, p1)) behind an optional
 * ACT, computed only where a following stride-`step` convolution reads it:
 *     a(i, j) = bias ? ACT(x(i, j), bias) : x(i, j)         inside the image, 0 outside
 *     y(i, j) = r( sum_{a, b < 4} k[a][b] a(i step + a - p0, j step + b - p0) )
 * for i < ho = ceil((h + p0 + p1 - 3) / step), j < wo = ceil((w + p0 + p1 - 3) / step).  The ResBlock uses
 * (p0, p1, step) = (2, 2, 1) in front of the 3x3 stride-2 conv (ho = h + 1) and (1, 1, 2) in front of the 1x1
 * stride-2 skip conv (ho = h / 2: only the even positions of the blurred image).
 *
 * fp32 summation order: separable.  Per input row the four column taps in ascending b,
 *     hsum = fma(a_3, 1, fma(a_2, 3, fma(a_1, 3, a_0)))
 * then the four rows in ascending a with the same weights and the same chain, then one product with 1/64
 * (exact) and the rounding.  With integer inputs every partial sum is exact.
 *
 * x: [n][h][w][ldx], frames x_ns apart; y: [n][ho][wo][ldy], frames y_ns apart; bias bf16 [c] or NULL.
 * c % 8 == 0; ldx, ldy >= c and multiples of 8; x_ns >= (h w - 1) ldx + c, y_ns >= (ho wo - 1) ldy + c, both
 * multiples of 8; p0, p1 in 0..3, step 1 or 2 (anything else VS_E_INVALID), h + p0 + p1 >= 4, w + p0 + p1 >= 4;
 * x, y, bias 16-byte aligned; y overlaps neither x nor bias.
 */
int vs_lrelu_blur(const void* x, long long x_ns, long long ldx, void* y, long long y_ns, long long ldy,
                  const void* bias, int n, int h, int w, int c, int p0, int p1, int step, void* stream);

/*
 * y = ACT(x, bias), and with skip != NULL the ResBlock tail (out + skip) / math.sqrt(2) on bf16 tensors:
 *     y = r( r(ACT(x, bias) + skip) * inv ),  inv = 1.0f / (float)sqrt(2.0)
 * torch on the device evaluates the division of a tensor by a host scalar as the product with the fp32
 * reciprocal of that scalar (its div_true kernel's scalar path), not as a division; this kernel does the same.
 *
 * x, skip, y: [n][npix][ld*] rows of c channels, frames *_ns apart.  y may be x (same pointer, ldy == ldx
 * and y_ns == x_ns); any other overlap of y with x, skip or bias is VS_E_INVALID.  c % 8 == 0; every ld >= c
 * and a multiple of 8; every ns >= (npix - 1) ld + c and a multiple of 8; all pointers 16-byte aligned.
 */
int vs_lrelu_merge(const void* x, long long x_ns, long long ldx, const void* bias, const void* skip,
                   long long s_ns, long long lds, void* y, long long y_ns, long long ldy, int n, long long npix,
                   int c, void* stream);

/*
 * Direction.forward (:589-591), a diag_embed matmul whose every output is one product rounded to bf16,
 * then a bf16 sum:  out[t][j] = r( sum_{i < m} r(alpha[t][i] * q[j][i]) ),  i ascending, t < rows, j < d.
 * alpha: rows of m values lda apart; q: d rows ldq apart (the QR basis, rounded to bf16); out rows ldo apart.
 * 1 <= m <= 32; lda, ldq >= m; ldo >= d; out overlaps neither alpha nor q.
 */
int vs_motion_direction(const void* alpha, long long lda, const void* q, long long ldq, void* out, long long ldo,
                        int rows, int d, int m, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VSTYLER_MOTION_H */
