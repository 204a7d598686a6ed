/*
 * libvstyler -- two modulation rows per sample (the Wan2.2-TI2V-5B DiT's image-to-video mode,
 * diffsynth/pipelines/wan_video_new.py:1339-1349, diffsynth/models/wan_video_dit.py:214-229, 262-265).
 *
 * With the clean first-frame latents fused into latent frame 0 the reference modulates every token of
 * that frame with timestep 0 and every other token with the step's timestep: a [1, S, 6, dim] tensor
 * that holds only two distinct rows.  Here the table keeps those two rows per sample and each row of
 * the activation picks one: row m of sample b = m / rows_per_batch is in segment
 * seg = ((m - b*rows_per_batch) >= seg_rows) and reads table row 2*b + seg.
 *
 * A fourth header of the same library and the same conventions as vstyler.h: bf16 raw 16-bit values,
 * launches on `stream`, no allocation, 0 (VS_OK) or a VS_E_* code, every shape / stride / alignment
 * violation rejected before anything is launched.  vs_abi_version() is unchanged (the entries are
 * additions) and they read no option.  The GEMM side of the same rule is vs_epilogue.seg_rows
 * (vstyler.h).
 */
#ifndef VSTYLER_SEG_H
#define VSTYLER_SEG_H

#include "vstyler.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * vs_layernorm_modulate with the modulation row 2*b + seg at shift / scale + index*mod_bstride.  The
 * arithmetic is that entry's: a row's output equals vs_layernorm_modulate's for that row with that
 * modulation row, bit for bit.  shift and scale are required, seg_rows >= 1 (seg_rows >=
 * rows_per_batch: every row is segment 0); dim, leading-dimension and alignment rules as
 * vs_layernorm_modulate.
 */
int vs_layernorm_modulate_seg(const void* x, long long ldx, void* out, long long ldo, int rows, int dim,
                              int rows_per_batch, int seg_rows, const void* shift, const void* scale,
                              long long mod_bstride, const void* weight, const void* bias, float eps, void* stream);

/*
 * vs_layernorm_modulate_fp8 with the same row choice: x8 / qscale equal vs_quant_fp8_rows of the rows
 * vs_layernorm_modulate_seg stores.
 */
int vs_layernorm_modulate_fp8_seg(const void* x, long long ldx, void* x8, long long ld8, float* qscale, int rows,
                                  int dim, int rows_per_batch, int seg_rows, const void* shift, const void* scale,
                                  long long mod_bstride, const void* weight, const void* bias, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VSTYLER_SEG_H */
