/*
 * libvstyler -- the image-conditioning entries (Wan I2V / FLF2V / Fun-InP: `y`, `clip_feature`).
 *
 * A second header of the same library and the same conventions as vstyler.h: bf16 raw 16-bit values,
 * row-major, launches on `stream`, no allocation, 0 (VS_OK) or a VS_E_* code, every shape / stride /
 * alignment violation rejected before anything is launched.  vs_abi_version() is unchanged (these
 * entries are additions) and no entry here reads an option of its own.
 */
#ifndef VSTYLER_IMAGE_H
#define VSTYLER_IMAGE_H

#include "vstyler.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The im2col of Conv3d(cx + cy, D, k=s=(1,2,2)) over cat([x, y], dim=1) without materialising the
 * cat (wan_video_new.py:1367-1368 + wan_video_dit.py:306-307): x [B or 1, cx, T, H, W],
 * y [B or 1, cy, T, H, W] -> tokens [B*T*(H/2)*(W/2)] rows of ld elements.  Row b*S+s gets column
 * c*4+kh*2+kw from x for c < cx and from y (channel c - cx) for cx <= c < cx+cy; columns
 * [4(cx+cy), ld) are written zero (the GEMM that follows needs K % 64 == 0: 36 channels give 144
 * columns in a 192-wide row, against a weight zero-padded to [D, 192]).  x_bs / y_bs: batch strides
 * in elements, 0 = one sample broadcast to every batch row.  cy = 0 (y may then be NULL) with
 * ld = 4 cx is vs_patchify.  VS_E_INVALID: a null pointer, a non-positive size, cx < 1, cy < 0, odd
 * height or width, ld % 8 != 0, ld < 4(cx+cy), x or y not 4-B aligned, tokens not 16-B aligned, a
 * negative or odd batch stride.
 */
int vs_patchify2(const void* x, long long x_bs, int cx, const void* y, long long y_bs, int cy, void* tokens,
                 long long ld, int batch, int frames, int height, int width, void* stream);

/*
 * out = bf16(gelu(float(x))), gelu(v) = 0.5 v (1 + erf(v / sqrt(2))): nn.GELU() of the image
 * embedding MLP (wan_video_dit.py:239), not the tanh form of VS_EPI_GELU.  n elements, any n >= 1;
 * out may be x.  VS_E_INVALID: a null pointer, n < 1, x or out not 2-B aligned.
 */
int vs_gelu_erf(const void* x, void* out, long long n, void* stream);

/*
 * o = bf16(o + bf16(softmax(q k^T * scale) v)): vs_attn_fwd's arguments and rules, the result added
 * to what o holds -- the image half of CrossAttention.forward (wan_video_dit.py:181-185: x = x + y
 * on bf16 tensors) without a second [sq, heads*128] buffer and an add pass.  Runs the checked
 * (online-softmax) 8-wave kernel alone: never the optimistic pass, whose redone items would add
 * twice, and never a split tail -- skv above 31 key tiles (1984 keys) is VS_E_UNSUPPORTED.
 * bsk = bsv = 0: one key set for every batch sample.  The bf16 attention value added is bit for
 * bit what vs_attn_fwd's checked kernel stores (VS_OPT_ATTN_NC 0, VS_OPT_ATTN_IMPL 8; the MFMA shape
 * follows VS_OPT_ATTN_MFMA).  o must not overlap q, k or v.
 */
int vs_attn_fwd_add(const void* q, const void* k, const void* v, void* o,
                    int batch, int sq, int skv, int heads, int head_dim,
                    long long ldq, long long ldk, long long ldv, long long ldo,
                    long long bsq, long long bsk, long long bsv, long long bso,
                    float scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VSTYLER_IMAGE_H */
