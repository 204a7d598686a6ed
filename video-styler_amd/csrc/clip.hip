// CLIP ViT-H/14 image encoder (include/vstyler_clip.h): the preprocessing + im2col kernel.  The tower
// itself runs on vs_gemm / vs_layernorm_modulate / vs_attn_fwd / vs_gelu_erf (vstyler/clip.py).
#include "common.h"
#include "../../include/vstyler_clip.h"

namespace {

constexpr int CLIP_PATCH = 14;
constexpr int CLIP_K = 3 * CLIP_PATCH * CLIP_PATCH;       // 588 columns of the im2col row
constexpr int CLIP_K_PAD = 640;                           // the next multiple of 64
constexpr int CLIP_MAX_SIZE = 64 * CLIP_PATCH;

// The four taps of output o on an axis of n_in source pixels resized to S: source coordinate
// ((2o+1) n_in - S) / (2S) as floor + remainder in integers, t = remainder / (2S) one fp32 division;
// cubic-convolution weights with A = -0.75 (the two polynomials of upsample_bicubic2d), every fp32
// operation rounded on its own; indices clamped to the border.
__device__ __forceinline__ void clip_taps(int o, int n_in, int S, int idx[4], float w[4]) {
#pragma clang fp contract(off)
    const long long den = 2LL * S;
    const long long num = (2LL * o + 1) * n_in - S;
    long long fl = num / den;
    long long rem = num - fl * den;
    if (rem < 0) {
        rem += den;
        fl -= 1;
    }
    const float t = __fdiv_rn((float)rem, (float)den);
    const float A = -0.75f;
    const float x0 = t + 1.0f, x1 = t, x2 = 1.0f - t, x3 = 2.0f - t;
    w[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
    w[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
    w[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
    w[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        long long i = fl - 1 + k;
        i = i < 0 ? 0 : (i > n_in - 1 ? n_in - 1 : i);
        idx[k] = (int)i;
    }
}

// one thread per (token row, 8 columns): 8 output pixels of 16 taps each, one 16-B store
__global__ __launch_bounds__(256) void clip_preprocess_kernel(const bf16_t* __restrict__ x, long long img_stride,
                                                              long long ch_stride, long long row_stride,
                                                              bf16_t* __restrict__ tok, long long ld, int H, int W,
                                                              int S, long long total) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int nch = (int)(ld >> 3), g = S / CLIP_PATCH;
    const int ch = (int)(i % nch);
    const long long row = i / nch;                  // (image, py, px)
    const int px = (int)(row % g), py = (int)((row / g) % g);
    const long long img = row / ((long long)g * g);
    const float mean[3] = {rbf(0.48145466f), rbf(0.4578275f), rbf(0.40821073f)};
    const float stdv[3] = {rbf(0.26862954f), rbf(0.26130258f), rbf(0.27577711f)};
    uint32_t o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int j = 8 * ch + e;
        o[e] = 0u;
        if (j >= CLIP_K) continue;
        const int c = j / (CLIP_PATCH * CLIP_PATCH), ky = (j / CLIP_PATCH) % CLIP_PATCH, kx = j % CLIP_PATCH;
        int iy[4], ix[4];
        float wy[4], wx[4];
        clip_taps(CLIP_PATCH * py + ky, H, S, iy, wy);
        clip_taps(CLIP_PATCH * px + kx, W, S, ix, wx);
        const bf16_t* plane = x + img * img_stride + c * ch_stride;
        float rowv[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const bf16_t* p = plane + iy[a] * row_stride;
            rowv[a] = bf2f(p[ix[0]]) * wx[0] + bf2f(p[ix[1]]) * wx[1] + bf2f(p[ix[2]]) * wx[2] + bf2f(p[ix[3]]) * wx[3];
        }
        const float r = rbf(rowv[0] * wy[0] + rowv[1] * wy[1] + rowv[2] * wy[2] + rowv[3] * wy[3]);
        const float u = rbf(rbf(0.5f * r) + 0.5f);
        o[e] = f2bf(__fdiv_rn(rbf(u - mean[c]), stdv[c]));
    }
    u32x4_t v = {o[0] | (o[1] << 16), o[2] | (o[3] << 16), o[4] | (o[5] << 16), o[6] | (o[7] << 16)};
    *reinterpret_cast<u32x4_t*>(tok + row * ld + 8 * ch) = v;
}

}  // namespace

extern "C" int vs_clip_preprocess(const void* x, long long img_stride, long long ch_stride, long long row_stride,
                                  void* tokens, long long ld, int n, int height, int width, int out_size,
                                  void* stream) {
    if (!x || !tokens || n <= 0 || height <= 0 || width <= 0) return VS_E_INVALID;
    if (out_size < CLIP_PATCH || out_size % CLIP_PATCH || out_size > CLIP_MAX_SIZE) return VS_E_INVALID;
    if (ld < CLIP_K_PAD || ld % 8 || (reinterpret_cast<uintptr_t>(tokens) & 15) ||
        (reinterpret_cast<uintptr_t>(x) & 1))
        return VS_E_INVALID;
    const long long plane = ((long long)height - 1) * row_stride + width;     // extent of one channel
    if (row_stride < width || ch_stride < plane || img_stride < 0 ||
        (img_stride > 0 && img_stride < 2 * ch_stride + plane))
        return VS_E_INVALID;
    const int g = out_size / CLIP_PATCH;
    const long long total = (long long)n * g * g * (ld / 8);
    if ((total + 255) / 256 > 0x7fffffffLL) return VS_E_INVALID;
    hipLaunchKernelGGL(clip_preprocess_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, (const bf16_t*)x, img_stride, ch_stride, row_stride, (bf16_t*)tokens, ld,
                       height, width, out_size, total);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
