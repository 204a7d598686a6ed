// Wan2.2-Animate's motion encoder (include/vstyler_motion.h): what runs between the convolutions of its
// StyleGAN2-style encoder -- the stem, FusedLeakyReLU fused into the 4x4 blur and into the ResBlock merge,
// and Direction.  Streaming VALU kernels: one lane per 16-byte chunk (8 channels) of a channels-last pixel,
// consecutive lanes on consecutive chunks, so a wave moves 1 KB of contiguous rows per access.
#include "common.h"
#include "../../include/vstyler_motion.h"

namespace {

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// byte ranges [a, a + na) and [b, b + nb) share a byte
inline bool overlaps(const void* a, long long na, const void* b, long long nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

__device__ __forceinline__ void unpack8(const u32x4_t& w, float* v) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = bflo(w[i]);
        v[2 * i + 1] = bfhi(w[i]);
    }
}
__device__ __forceinline__ u32x4_t pack8(const float* v) {
    u32x4_t w;
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = pack2(v[2 * i], v[2 * i + 1]);
    return w;
}

constexpr float ACT_S2 = 1.41421353816986083984375f;       // (float)2**0.5
constexpr float MERGE_INV = 1.0f / ACT_S2;                  // 1.0f / (float)sqrt(2.0), an fp32 division

// fused_leaky_relu on bf16 tensors: the add, the leaky ReLU and the product each materialise a bf16 tensor
__device__ __forceinline__ float act(float x, float b) {
    const float a = rbf(x + b);
    return rbf(rbf(a >= 0.f ? a : a * 0.2f) * ACT_S2);
}

// one lane per (pixel, 8 output channels)
__global__ __launch_bounds__(256) void motion_stem_kernel(const void* __restrict__ x, int x_u8,
                                                          const bf16_t* __restrict__ wt,
                                                          const bf16_t* __restrict__ bias, bf16_t* __restrict__ y,
                                                          long long y_ns, long long ldy, long long plane, int cg,
                                                          long long total, long long nplane) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int g = (int)(i % cg);
    const long long pix = i / cg;                             // f * plane + p
    float px[3];
    if (x_u8) {
        const uint8_t* u = reinterpret_cast<const uint8_t*>(x) + pix * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) px[k] = rbf(rbf((float)u[k] * (2.0f / 255.0f)) + -1.0f);
    } else {
        const bf16_t* b = reinterpret_cast<const bf16_t*>(x) + pix;
#pragma unroll
        for (int k = 0; k < 3; ++k) px[k] = bf2f(b[k * nplane]);
    }
    float wv[24], bv[8], o[8];
    const u32x4_t* wp = reinterpret_cast<const u32x4_t*>(wt + g * 24);
    unpack8(wp[0], wv);
    unpack8(wp[1], wv + 8);
    unpack8(wp[2], wv + 16);
    unpack8(*reinterpret_cast<const u32x4_t*>(bias + g * 8), bv);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float c = rbf(fmaf(px[2], wv[3 * e + 2], fmaf(px[1], wv[3 * e + 1], px[0] * wv[3 * e])));
        o[e] = act(c, bv[e]);
    }
    const long long f = pix / plane, p = pix % plane;
    *reinterpret_cast<u32x4_t*>(y + f * y_ns + p * ldy + g * 8) = pack8(o);
}

constexpr int BL_RT = 16;       // output rows per lane: the 4-row window rolls down a column strip

// One horizontally filtered input row at this lane's output column: taps b = 0..3 at columns c0 + b.
template <bool ACT>
__device__ __forceinline__ void blur_hrow(const bf16_t* __restrict__ xf, long long ldx, int row, int h, int w, int c0,
                                          const float* bv, float* hs) {
#pragma unroll
    for (int e = 0; e < 8; ++e) hs[e] = 0.f;
    if (row < 0 || row >= h) return;
    const bf16_t* xr = xf + (long long)row * w * ldx;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int col = c0 + b;
        float a[8];
        if (col >= 0 && col < w) {
            unpack8(*reinterpret_cast<const u32x4_t*>(xr + (long long)col * ldx), a);
            if (ACT) {
#pragma unroll
                for (int e = 0; e < 8; ++e) a[e] = act(a[e], bv[e]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] = 0.f;
        }
        const float k = (b == 0 || b == 3) ? 1.f : 3.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) hs[e] = b == 0 ? a[e] : fmaf(a[e], k, hs[e]);
    }
}

// one lane per (frame, strip of BL_RT output rows, output column, 8 channels)
template <bool ACT, int STEP>
__global__ __launch_bounds__(256) void lrelu_blur_kernel(const bf16_t* __restrict__ x, long long x_ns, long long ldx,
                                                         bf16_t* __restrict__ y, long long y_ns, long long ldy,
                                                         const bf16_t* __restrict__ bias, int h, int w, int ho, int wo,
                                                         int cg, int p0, int nstrip, long long total) {
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int g = (int)(i % cg);
    i /= cg;
    const int j = (int)(i % wo);
    i /= wo;
    const int strip = (int)(i % nstrip);
    const long long f = i / nstrip;
    float bv[8];
    if (ACT) unpack8(*reinterpret_cast<const u32x4_t*>(bias + g * 8), bv);
    const bf16_t* xf = x + f * x_ns + g * 8;
    bf16_t* yf = y + f * y_ns + g * 8;
    const int i0 = strip * BL_RT, i1 = min(i0 + BL_RT, ho);
    const int c0 = j * STEP - p0;
    int row = i0 * STEP - p0;                                 // the window's first input row
    float hw[4][8];
#pragma unroll
    for (int a = 0; a < 4; ++a) blur_hrow<ACT>(xf, ldx, row + a, h, w, c0, bv, hw[a]);
    for (int io = i0; io < i1; ++io) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
            o[e] = fmaf(hw[3][e], 1.f, fmaf(hw[2][e], 3.f, fmaf(hw[1][e], 3.f, hw[0][e]))) * (1.0f / 64.0f);
        *reinterpret_cast<u32x4_t*>(yf + ((long long)io * wo + j) * ldy) = pack8(o);
        if (io + 1 < i1) {
#pragma unroll
            for (int s = 0; s < STEP; ++s) {
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int e = 0; e < 8; ++e) hw[a][e] = hw[a + 1][e];
                blur_hrow<ACT>(xf, ldx, row + 4 + s, h, w, c0, bv, hw[3]);
            }
            row += STEP;
        }
    }
}

// one lane per 16-byte chunk; x and y are not __restrict__: y may be x (each lane reads its chunk first)
template <bool SKIP>
__global__ __launch_bounds__(256) void lrelu_merge_kernel(const bf16_t* x, long long x_ns, long long ldx,
                                                          const bf16_t* __restrict__ bias,
                                                          const bf16_t* __restrict__ skip, long long s_ns, long long lds,
                                                          bf16_t* y, long long y_ns, long long ldy, long long npix, int cg,
                                                          long long total) {
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int g = (int)(i % cg);
    i /= cg;
    const long long p = i % npix, f = i / npix;
    float v[8], bv[8], s[8];
    unpack8(*reinterpret_cast<const u32x4_t*>(x + f * x_ns + p * ldx + g * 8), v);
    unpack8(*reinterpret_cast<const u32x4_t*>(bias + g * 8), bv);
    if (SKIP) unpack8(*reinterpret_cast<const u32x4_t*>(skip + f * s_ns + p * lds + g * 8), s);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        v[e] = act(v[e], bv[e]);
        if (SKIP) v[e] = rbf(v[e] + s[e]) * MERGE_INV;
    }
    *reinterpret_cast<u32x4_t*>(y + f * y_ns + p * ldy + g * 8) = pack8(v);
}

// one lane per output element; m <= 32 products in ascending i
__global__ __launch_bounds__(256) void motion_direction_kernel(const bf16_t* __restrict__ alpha, long long lda,
                                                               const bf16_t* __restrict__ q, long long ldq,
                                                               bf16_t* __restrict__ out, long long ldo, int d, int m,
                                                               long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int j = (int)(i % d);
    const long long t = i / d;
    const bf16_t* ar = alpha + t * lda;
    const bf16_t* qr = q + (long long)j * ldq;
    float s = 0.f;
    for (int k = 0; k < m; ++k) s += rbf(bf2f(ar[k]) * bf2f(qr[k]));
    out[t * ldo + j] = (bf16_t)f2bf(s);
}

// a [n][rows][ld] tensor of c-wide rows: stride rules and its extent in bytes
inline bool frames_ok(long long ns, long long ld, long long rows, int c) {
    return ld >= c && !(ld & 7) && !(ns & 7) && ns >= (rows - 1) * ld + c;
}
inline long long frames_bytes(long long ns, long long ld, long long rows, int c, int n) {
    return ((n - 1) * ns + (rows - 1) * ld + c) * 2;
}

}  // namespace

extern "C" int vs_motion_stem(const void* x, int x_u8, const void* wt, const void* bias, void* y, long long y_ns,
                              long long ldy, int n, int h, int w, int c0, void* stream) {
    if (!x || !wt || !bias || !y || n <= 0 || h <= 0 || w <= 0 || c0 <= 0 || c0 % 8 || c0 > 512) return VS_E_INVALID;
    const long long plane = (long long)h * w;
    if (!frames_ok(y_ns, ldy, plane, c0)) return VS_E_INVALID;
    if (!al16(wt) || !al16(bias) || !al16(y) || (!x_u8 && (reinterpret_cast<uintptr_t>(x) & 1))) return VS_E_INVALID;
    const long long nplane = (long long)n * plane;
    const long long y_bytes = frames_bytes(y_ns, ldy, plane, c0, n);
    if (overlaps(y, y_bytes, x, nplane * 3 * (x_u8 ? 1 : 2)) || overlaps(y, y_bytes, wt, c0 * 6LL) ||
        overlaps(y, y_bytes, bias, c0 * 2LL))
        return VS_E_INVALID;
    const int cg = c0 / 8;
    const long long total = nplane * cg, blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return VS_E_INVALID;
    hipLaunchKernelGGL(motion_stem_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, x_u8,
                       (const bf16_t*)wt, (const bf16_t*)bias, (bf16_t*)y, y_ns, ldy, plane, cg, total, nplane);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_lrelu_blur(const void* x, long long x_ns, long long ldx, void* y, long long y_ns, long long ldy,
                             const void* bias, int n, int h, int w, int c, int p0, int p1, int step, void* stream) {
    if (!x || !y || n <= 0 || h <= 0 || w <= 0 || c <= 0 || c % 8) return VS_E_INVALID;
    if (p0 < 0 || p0 > 3 || p1 < 0 || p1 > 3 || (step != 1 && step != 2)) return VS_E_INVALID;
    if (h + p0 + p1 < 4 || w + p0 + p1 < 4) return VS_E_INVALID;
    const int ho = (h + p0 + p1 - 3 + step - 1) / step, wo = (w + p0 + p1 - 3 + step - 1) / step;
    if (!frames_ok(x_ns, ldx, (long long)h * w, c) || !frames_ok(y_ns, ldy, (long long)ho * wo, c)) return VS_E_INVALID;
    if (!al16(x) || !al16(y) || !al16(bias)) return VS_E_INVALID;
    const long long y_bytes = frames_bytes(y_ns, ldy, (long long)ho * wo, c, n);
    if (overlaps(y, y_bytes, x, frames_bytes(x_ns, ldx, (long long)h * w, c, n)) ||
        (bias && overlaps(y, y_bytes, bias, c * 2LL)))
        return VS_E_INVALID;
    const int cg = c / 8, nstrip = (ho + BL_RT - 1) / BL_RT;
    const long long total = (long long)n * nstrip * wo * cg, blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return VS_E_INVALID;
#define VS_BLUR(A, S)                                                                                              \
    hipLaunchKernelGGL((lrelu_blur_kernel<A, S>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,      \
                       (const bf16_t*)x, x_ns, ldx, (bf16_t*)y, y_ns, ldy, (const bf16_t*)bias, h, w, ho, wo, cg, \
                       p0, nstrip, total)
    if (bias) {
        if (step == 1) VS_BLUR(true, 1); else VS_BLUR(true, 2);
    } else {
        if (step == 1) VS_BLUR(false, 1); else VS_BLUR(false, 2);
    }
#undef VS_BLUR
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_lrelu_merge(const void* x, long long x_ns, long long ldx, const void* bias, const void* skip,
                              long long s_ns, long long lds, void* y, long long y_ns, long long ldy, int n,
                              long long npix, int c, void* stream) {
    if (!x || !bias || !y || n <= 0 || npix <= 0 || c <= 0 || c % 8) return VS_E_INVALID;
    if (!frames_ok(x_ns, ldx, npix, c) || !frames_ok(y_ns, ldy, npix, c) || (skip && !frames_ok(s_ns, lds, npix, c)))
        return VS_E_INVALID;
    if (!al16(x) || !al16(bias) || !al16(skip) || !al16(y)) return VS_E_INVALID;
    const long long y_bytes = frames_bytes(y_ns, ldy, npix, c, n);
    if (!(x == y && ldx == ldy && x_ns == y_ns) && overlaps(y, y_bytes, x, frames_bytes(x_ns, ldx, npix, c, n)))
        return VS_E_INVALID;
    if (overlaps(y, y_bytes, bias, c * 2LL) || (skip && overlaps(y, y_bytes, skip, frames_bytes(s_ns, lds, npix, c, n))))
        return VS_E_INVALID;
    const int cg = c / 8;
    const long long total = (long long)n * npix * cg, blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return VS_E_INVALID;
    if (skip)
        hipLaunchKernelGGL(lrelu_merge_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)x, x_ns, ldx, (const bf16_t*)bias, (const bf16_t*)skip, s_ns, lds, (bf16_t*)y,
                           y_ns, ldy, npix, cg, total);
    else
        hipLaunchKernelGGL(lrelu_merge_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)x, x_ns, ldx, (const bf16_t*)bias, (const bf16_t*)nullptr, 0LL, 0LL, (bf16_t*)y,
                           y_ns, ldy, npix, cg, total);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_motion_direction(const void* alpha, long long lda, const void* q, long long ldq, void* out,
                                   long long ldo, int rows, int d, int m, void* stream) {
    if (!alpha || !q || !out || rows <= 0 || d <= 0 || m < 1 || m > 32 || lda < m || ldq < m || ldo < d)
        return VS_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(alpha) | reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(out)) & 1)
        return VS_E_INVALID;
    const long long o_bytes = (((long long)rows - 1) * ldo + d) * 2;
    if (overlaps(out, o_bytes, alpha, (((long long)rows - 1) * lda + m) * 2) ||
        overlaps(out, o_bytes, q, (((long long)d - 1) * ldq + m) * 2))
        return VS_E_INVALID;
    const long long total = (long long)rows * d, blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return VS_E_INVALID;
    hipLaunchKernelGGL(motion_direction_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)alpha, lda, (const bf16_t*)q, ldq, (bf16_t*)out, ldo, d, m, total);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
