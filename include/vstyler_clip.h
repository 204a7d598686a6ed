/*
 * libvstyler -- the CLIP ViT-H/14 image encoder's entry (WanImageEncoder.encode_image,
 * diffsynth/models/wan_video_image_encoder.py:852-880: the clip_feature of Wan I2V / FLF2V / Fun-InP).
 *
 * A third header of the same library and the same conventions as vstyler.h and vstyler_image.h: bf16
 * raw 16-bit values, launches on `stream`, no allocation, 0 (VS_OK) or a VS_E_* code, every shape /
 * stride / alignment violation rejected before anything is launched.  vs_abi_version() is unchanged
 * (the entry is an addition) and it reads no option.  Everything else of the tower runs on entries of
 * the other two headers (vs_gemm, vs_layernorm_modulate, vs_attn_fwd, vs_gelu_erf).
 */
#ifndef VSTYLER_CLIP_H
#define VSTYLER_CLIP_H

#include "vstyler.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * encode_image's preprocessing and the im2col of the patch convolution in one launch:
 *   F.interpolate(u, (S, S), mode='bicubic', align_corners=False)            (:868-872)
 *   .mul_(0.5).add_(0.5), Normalize(mean, std)                               (:874)
 *   Conv2d(3, dim, k=14, s=14)'s patches                                     (:460)
 * x: n images of 3 channels, height x width, bf16 in [-1, 1]; pixel (c, r, q) of image i at element
 * i*img_stride + c*ch_stride + r*row_stride + q (a (1, 3, 1, H, W) frame is read in place with
 * ch_stride = H*W, row_stride = W; img_stride 0 repeats one image).  S = out_size (224 for ViT-H/14),
 * g = S / 14 patches per side.  tokens: [n*g*g] rows of ld elements; column c*196 + ky*14 + kx of row
 * i*g*g + py*g + px is the normalised pixel (c, 14 py + ky, 14 px + kx); columns [588, ld) are written
 * zero (the GEMM that follows needs K % 64 == 0: 588 pads to 640 against a patch weight zero-padded to
 * [dim, 640]).
 *
 * Arithmetic.  The source coordinate of output o on an axis of n_in pixels is the exact rational
 * ((2o+1) n_in - S) / (2S): floor and remainder in integers, the fraction t one fp32 division.  The
 * four cubic-convolution weights (A = -0.75) of t, the four row sums and their sum over the rows are
 * fp32, one operation at a time (no contraction), tap indices clamped to the border; no antialias.
 * Then the reference's five bf16 roundings in its order: r = bf16(sum), bf16(0.5 r), bf16(. + 0.5),
 * bf16(. - bf16(mean[c])), bf16(. / bf16(std[c])) with an IEEE fp32 division, mean = (0.48145466,
 * 0.4578275, 0.40821073), std = (0.26862954, 0.26130258, 0.27577711).
 * (torch evaluates the coordinate as scale*(o + 0.5) - 0.5 in fp32; the exact rational differs from it
 * by less than a bf16 ulp of the interpolated value: DESIGN.md section 7.)
 *
 * Any height, width >= 1.  VS_E_INVALID: a null pointer, n / height / width < 1, out_size < 14 or not
 * a multiple of 14 or above 896, ld < 640, ld % 8 != 0, tokens not 16-B aligned, x not 2-B aligned,
 * row_stride < width, ch_stride < (height-1)*row_stride + width, img_stride negative or (non-zero and)
 * below 2*ch_stride + (height-1)*row_stride + width.
 */
int vs_clip_preprocess(const void* x, long long img_stride, long long ch_stride, long long row_stride,
                       void* tokens, long long ld, int n, int height, int width, int out_size, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VSTYLER_CLIP_H */
