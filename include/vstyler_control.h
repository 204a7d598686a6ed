/*
 * libvstyler -- Wan-Fun control: the reference-image tokens of a has_ref_conv DiT and the camera
 * control adapter's input (diffsynth/pipelines/wan_video_new.py:777-845, 1384-1390, 1463-1466,
 * diffsynth/models/wan_video_dit.py:339-345, diffsynth/models/wan_video_camera_controller.py).
 *
 * A fifth header of the same library and the same conventions as vstyler.h: bf16 raw 16-bit values,
 * launches on `stream`, no allocation, 0 (VS_OK) or a VS_E_* code, every shape / stride / alignment
 * violation rejected before anything is launched.  vs_abi_version() is unchanged (the entries are
 * additions) and they read no option.
 */
#ifndef VSTYLER_CONTROL_H
#define VSTYLER_CONTROL_H

#include "vstyler.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The reference tokens in front of every sample's rows: dst is [batch * (n + s), dim] rows ldd apart;
 * rows [b (n + s), b (n + s) + n) of sample b become src rows [0, n) of sample b (src rows dim apart,
 * samples src_bs elements apart; src_bs 0: one token set for every sample).  No other row of dst is
 * touched.  dim % 8 == 0, ldd % 8 == 0, ldd >= dim, src_bs 0 or >= n dim and a multiple of 8; src and
 * dst 16-byte aligned.
 */
int vs_ref_rows(const void* src, long long src_bs, void* dst, long long ldd, int batch, int n, int s, int dim,
                void* stream);

/*
 * vs_unpatchify whose sample b reads its frames * (height / 2) * (width / 2) token rows from row
 * b (skip + S) + skip of `tokens` (rows of 4 channels values): the rows behind `skip` prepended ones.
 * skip 0 is vs_unpatchify, bit for bit.  skip >= 0; the other rules are vs_unpatchify's.
 */
int vs_unpatchify_skip(const void* tokens, void* lat, int batch, int channels, int frames, int height, int width,
                       int skip, void* stream);

/*
 * The camera adapter's input, bf16 [24, t, height, width]: channel c 4 + j of latent frame tt is
 * component c of the Pluecker ray (moment o x d, direction d) of pixel frame max(0, 4 tt + j - 3)
 * (the first frame four times, then groups of four).  intrinsics: fp32 [frames, 4] = (fx W, fy H, cx W,
 * cy H) per pixel frame; c2w: fp32 [frames, 12], the relative camera-to-world 3 x 4, row major.  The ray
 * of pixel (x, y): u = ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1) normalised, d = R u, o = the
 * matrix's last column; fp32 arithmetic, one rounding to bf16.  frames >= 4 t - 3; out 2-byte,
 * intrinsics / c2w 4-byte aligned.
 */
int vs_camera_rays(const float* intrinsics, const float* c2w, void* out, int frames, int t, int height, int width,
                   void* stream);

/*
 * PixelUnshuffle(8) + the unfold of a 2x2 / stride 2 convolution: in bf16 [channels, t, height, width]
 * -> out [t (height / 16) (width / 16), 256 channels], rows ldo apart.  Column
 * (c 64 + dy 8 + dx) 4 + kh 2 + kw of row (tt, oy, ox) is pixel ((2 oy + kh) 8 + dy, (2 ox + kw) 8 + dx)
 * of in[c][tt].  height, width multiples of 16; ldo >= 256 channels, ldo % 8 == 0; in and out 16-byte
 * aligned.
 */
int vs_camera_im2col(const void* in, void* out, long long ldo, int channels, int t, int height, int width,
                     void* stream);

/*
 * x = max(x, 0) on n bf16 values in place, with torch.relu's bits on the device: every x <= 0 becomes +0
 * (-0 too), a NaN stays.  n % 8 == 0, x 16-byte aligned.
 */
int vs_relu(void* x, long long n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VSTYLER_CONTROL_H */
