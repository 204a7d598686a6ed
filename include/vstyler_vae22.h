/*
 * libvstyler -- the Wan2.2 VAE (WanVideoVAE38: 48 latent channels, stride 16; diffsynth/models/
 * wan_video_vae.py:199-265, 345-514, 620-733, 842-940, 1269-1382): what it needs beside the Wan2.1 VAE's
 * entries (vs_vae_conv and the tile kernels of vstyler.h) -- the 2x2 pixel patchify and its inverse, the
 * parameter-free shortcuts of Down_ResidualBlock / Up_ResidualBlock, the channel RMS norm at the decoder's
 * widths, and the attention softmax that keeps its probabilities as a bf16 hi / lo pair.
 *
 * A sixth header of the same library and the same conventions as vstyler.h: bf16 raw 16-bit values,
 * activations channels-last [n, t, h, w, c], launches on `stream`, no allocation, 0 (VS_OK) or a VS_E_*
 * code, every pointer / shape / stride / alignment violation rejected before anything is launched.
 * vs_abi_version() is unchanged (the entries are additions) and they read no option.
 */
#ifndef VSTYLER_VAE22_H
#define VSTYLER_VAE22_H

#include "vstyler.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * vs_vae_rmsnorm for wider rows: y = x / max(||x||, 1e-12) * sqrt(c) * gamma (+ SiLU) over the c channels
 * of each of npix pixels (rows ldx / ldy elements apart; y may be x).  The same arithmetic: the norm
 * rounded to bf16, one reciprocal per pixel, three bf16-rounded multiplies, SiLU as
 * v * rcp(1 + exp2(-v log2 e)).  c % 32 == 0, c <= 1024; ldx, ldy >= c and multiples of 8; x, y, gamma
 * 16-byte aligned.
 */
int vs_vae22_rmsnorm(const void* x, long long ldx, void* y, long long ldy, const void* gamma, long long npix,
                     int c, int silu, void* stream);

/*
 * y += AvgDown3D(x) (wan_video_vae.py:345-395), whole-sequence form, in place on
 * y [n, t_out, h_in / fs, w_in / fs, c_out]; x [n, t_in, h_in, w_in, c_in], both contiguous.  With
 * F = ft fs fs and g = c_in F / c_out, output channel o is the mean over i < g of flat index f = o g + i:
 * input channel f / F at time offset it = (f % F) / (fs fs), row offset ih = (f % F) / fs % fs, column
 * offset iw = f % fs.  ft 1: t_out = t_in, frame j reads frame j.  ft 2: t_out = 1 + (t_in - 1) / 2, frame j
 * reads frames 2 j - 1 (it 0; frame -1 is zero) and 2 j (it 1).  The mean is an fp32 sum divided by g and
 * rounded to bf16 once, the add is rounded once.  ft, fs in {1, 2}; c_in F % c_out == 0; c_in % 8 == 0,
 * c_out % 8 == 0; t_in odd when ft is 2; h_in, w_in multiples of fs; x and y 16-byte aligned.
 */
int vs_vae22_avgdown_add(const void* x, void* y, int n, int t_in, int h_in, int w_in, int c_in, int c_out, int ft,
                         int fs, void* stream);

/*
 * y += DupUp3D(x) (wan_video_vae.py:398-439, first_chunk on the first frame), whole-sequence form, in
 * place on y [n, ft (t_in - 1) + 1, fs h_in, fs w_in, c_out]; x [n, t_in, h_in, w_in, c_in], both contiguous.
 * With F = ft fs fs and r = c_out F / c_in, output (o, frame tau, row yy, column xx) reads input channel
 * (o F + it fs fs + (yy % fs) fs + xx % fs) / r of frame (tau + ft - 1) / ft, it = (tau + ft - 1) % ft, pixel
 * (yy / fs, xx / fs).  One rounding, of the add.  ft, fs in {1, 2}; c_out F % c_in == 0; c_in % 8 == 0,
 * c_out % 8 == 0; x and y 16-byte aligned.
 */
int vs_vae22_dupup_add(const void* x, void* y, int n, int t_in, int h_in, int w_in, int c_in, int c_out, int ft,
                       int fs, void* stream);

/*
 * patchify(x, 2) (wan_video_vae.py:199-211, "b c f (h q) (w r) -> b (c r q) f h w") on channels-last frames:
 * src [nt, h, w, ld_src] with RGB in channels 0-2 -> dst [nt, h / 2, w / 2, 32]; channel 4 c + 2 r + q of
 * dst pixel (y, x) is src[2 y + q, 2 x + r, c], channels 12-31 are written as zero (the conv kernel's
 * 32-channel input block).  h, w even; ld_src >= 4 and a multiple of 4; src 8-byte, dst 16-byte aligned.
 */
int vs_vae22_patchify(const void* src, long long ld_src, void* dst, int nt, int h, int w, void* stream);

/*
 * unpatchify(x, 2) (wan_video_vae.py:214-224), the inverse: src [nt, h, w, ld_src] with the 12 channels
 * first -> dst [nt, 2 h, 2 w, 4]; channel c < 3 of dst pixel (2 y + q, 2 x + r) is src[y, x, 4 c + 2 r + q],
 * channel 3 is written as zero.  ld_src >= 12 and a multiple of 4; src 8-byte, dst 16-byte aligned.
 */
int vs_vae22_unpatchify(const void* src, long long ld_src, void* dst, int nt, int h, int w, void* stream);

/*
 * Row softmax of fp32 attention scores (vs_vae_softmax's arithmetic: row max, expf, one reciprocal) with each
 * probability kept as the bf16 pair hi = bf16(p), lo = bf16(p - hi): s [rows, ncols] fp32, rows ld_s apart ->
 * p [rows, ld_p] bf16, hi at column j and lo at column ld_p / 2 + j for j < ncols, zero in the other columns of
 * both halves.  One bf16 GEMM over K = ld_p against V^T laid out twice then accumulates hi V + lo V in fp32:
 * P to about 16 bits, where vs_vae_softmax rounds it to 8.  ld_s >= ncols; ld_p even, ld_p / 2 >= ncols; s
 * 4-byte, p 2-byte aligned.
 */
int vs_vae22_softmax_split(const float* s, long long ld_s, void* p, long long ld_p, long long rows, int ncols,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VSTYLER_VAE22_H */
