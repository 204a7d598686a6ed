/*
 * libvstyler -- Wan2.2-Animate: the face adapter's per-frame cross-attention and the row operators of its
 * once-per-call preparation (diffsynth/models/wan_video_animate_adapter.py: FaceBlock, FaceEncoder, RMSNorm).
 *
 * A seventh header of the same library and the same conventions as vstyler.h: bf16 raw 16-bit values,
 * launches on `stream`, no allocation, 0 (VS_OK) or a VS_E_* code, every shape / stride / alignment
 * violation rejected before anything is launched.  vs_abi_version() is unchanged (the entries are
 * additions) and they read no option.
 *
 * The per-head RMSNorm of both entries below is one device function with the reference RMSNorm's two
 * roundings over the head's 128 columns: n = bf16(x * rsqrt(mean_128(x^2) + eps)), y = bf16(n * w[c]),
 * the mean and the products in fp32.
 */
#ifndef VSTYLER_ANIMATE_H
#define VSTYLER_ANIMATE_H

#include "vstyler.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * FaceBlock's attention: every token row attends the nkeys motion tokens of its own latent frame.
 *
 * q: [batch * rows_per_batch] rows ldq apart, `heads` heads of 128 columns each; row r belongs to sample
 * b = r / rows_per_batch and to token t = r % rows_per_batch + token_offset of that sample, i.e. to frame
 * f = t / tokens_per_frame.  k, v: row (f nkeys + j) of sample b is key / value j of frame f, rows ldkv
 * apart, samples kv_bs elements apart (0: one set for every sample); k is already normalised.  Per
 * (row, head):
 *     qn  = the per-head RMSNorm of q with weight wq[0..127] (two roundings, above);
 *     s_j = scale * sum_c qn[c] k_j[c]     fp32, j < nkeys: each lane's 8 columns by fused multiply-add in
 *           column order, the 16 partial sums pairwise (lane pairs, quads, halves, the row), one product;
 *     p_j = exp(s_j - max_j s_j), l = sum_j p_j     fp32, p never rounded to bf16, q never pre-scaled;
 *     o   = bf16((sum_j p_j v_j) * (1 / l))         the sums in key order, the reciprocal in fp32.
 * Rows with t >= frames * tokens_per_frame (the pad rows of a sequence-parallel split) get zeros.  Columns
 * of o outside [0, heads * 128) are not written.  o may be q itself (same pointer and ldo == ldq); any other
 * overlap of o with q, k, v or wq is VS_E_INVALID.
 *
 * head_dim != 128: VS_E_UNSUPPORTED.  1 <= nkeys <= 8; ldq, ldo, ldkv >= heads * 128 and multiples of 8;
 * kv_bs 0 or >= (frames * nkeys - 1) * ldkv + heads * 128 and a multiple of 8; token_offset >= 0; eps >= 0;
 * scale finite; q, k, v, o, wq 16-byte aligned.
 */
int vs_face_attn(const void* q, long long ldq, const void* k, const void* v, long long ldkv, long long kv_bs,
                 void* o, long long ldo, const void* wq, int batch, int rows_per_batch, int heads, int head_dim,
                 int frames, int tokens_per_frame, int nkeys, int token_offset, float eps, float scale,
                 void* stream);

/*
 * The per-head RMSNorm (above) in place on `heads` heads of 128 columns of every row of x (rows ldx apart);
 * columns outside the heads keep their bits.  The same device function as vs_face_attn's qn: bit-identical
 * to it.  head_dim != 128: VS_E_UNSUPPORTED.  ldx >= heads * 128 and a multiple of 8; eps >= 0; x and w
 * 16-byte aligned.
 */
int vs_head_rmsnorm(void* x, long long ldx, int rows, int heads, int head_dim, const void* w, float eps,
                    void* stream);

/*
 * out = bf16(silu(h)), h = bf16(LayerNorm(x)) without affine (fp32 statistics, eps) when norm != 0 and
 * h = x when norm == 0; silu(h) = h / (1 + exp(-h)) evaluated in double with one rounding to bf16.  rows of
 * dim columns, x rows ldx and out rows ldo apart; out may be x (same pointer and ldo == ldx).  dim % 8 == 0,
 * dim <= 8192; ldx, ldo >= dim and multiples of 8; eps >= 0; x and out 16-byte aligned.
 */
int vs_ln_silu(const void* x, long long ldx, void* out, long long ldo, int rows, int dim, int norm, float eps,
               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VSTYLER_ANIMATE_H */
