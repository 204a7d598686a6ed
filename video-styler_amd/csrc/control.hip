// Wan-Fun control (include/vstyler_control.h): the reference-image rows in front of every sample's
// tokens, the unpatchify that skips them, and the camera adapter's input (Pluecker rays, grouped in
// fours) and its PixelUnshuffle(8) + 2x2/2 unfold.  Data movement and one-off per-call work: one thread
// per 16-byte chunk or per pixel, plain vector stores, bounds from `total` alone.
#include "common.h"
#include "../../include/vstyler_control.h"

namespace {

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// blocks of 256 threads for `total` items, 0 when that does not fit a launch
inline unsigned nblk256(long long total) {
    const long long b = (total + 255) / 256;
    return b > 0x7fffffffLL ? 0u : (unsigned)b;
}

// one thread per 16-byte chunk of a reference row of one sample
__global__ __launch_bounds__(256) void ref_rows_kernel(const bf16_t* __restrict__ src, long long src_bs,
                                                       bf16_t* __restrict__ dst, long long ldd, int n, int s,
                                                       int nch, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ch = (int)(i % nch);
    const long long r = i / nch;             // (b, row)
    const int row = (int)(r % n);
    const long long b = r / n;
    const u32x4_t v = *reinterpret_cast<const u32x4_t*>(src + b * src_bs + ((long long)row * nch + ch) * 8);
    *reinterpret_cast<u32x4_t*>(dst + (b * ((long long)n + s) + row) * ldd + 8LL * ch) = v;
}

// unpatchify_kernel of elementwise.hip with sample b's rows starting at b (skip + S) + skip
__global__ __launch_bounds__(256) void unpatchify_skip_kernel(const bf16_t* __restrict__ tok, bf16_t* __restrict__ lat,
                                                              int C, int T, int H, int W, long long skip,
                                                              long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int h2 = H >> 1, w2 = W >> 1;
    const int ww = (int)(i % w2);
    const int hh = (int)((i / w2) % h2);
    const int f = (int)((i / ((long long)w2 * h2)) % T);
    const int c = (int)((i / ((long long)w2 * h2 * T)) % C);
    const long long b = i / ((long long)w2 * h2 * T * C);
    const long long S = (long long)T * h2 * w2;
    const long long t = b * (skip + S) + skip + ((long long)f * h2 + hh) * w2 + ww;
    const bf16_t* src = tok + t * (4LL * C) + c;
    bf16_t* dst = lat + (((b * C + c) * T + f) * H + 2 * hh) * (long long)W + 2 * ww;
    const uint32_t top = (uint32_t)src[0] | ((uint32_t)src[C] << 16);
    const uint32_t bot = (uint32_t)src[2 * C] | ((uint32_t)src[3 * C] << 16);
    *reinterpret_cast<uint32_t*>(dst) = top;
    *reinterpret_cast<uint32_t*>(dst + W) = bot;
}

// one thread per (latent frame tt, slot j, pixel): the ray of pixel frame max(0, 4 tt + j - 3), its six
// components to channels c 4 + j
__global__ __launch_bounds__(256) void camera_rays_kernel(const float* __restrict__ intr, const float* __restrict__ c2w,
                                                          bf16_t* __restrict__ out, int T, int H, int W,
                                                          long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % W);
    const int y = (int)((i / W) % H);
    const int j = (int)((i / ((long long)W * H)) % 4);
    const int tt = (int)(i / ((long long)W * H * 4));
    const int fr = max(0, 4 * tt + j - 3);
    const float* k = intr + 4LL * fr;
    const float* m = c2w + 12LL * fr;
    const float ux = ((float)x + 0.5f - k[2]) / k[0];
    const float uy = ((float)y + 0.5f - k[3]) / k[1];
    const float nrm = sqrtf(ux * ux + uy * uy + 1.0f);
    const float dx = ux / nrm, dy = uy / nrm, dz = 1.0f / nrm;
    float d[3], o[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        d[r] = dx * m[4 * r] + dy * m[4 * r + 1] + dz * m[4 * r + 2];
        o[r] = m[4 * r + 3];
    }
    float v[6];
    v[0] = o[1] * d[2] - o[2] * d[1];
    v[1] = o[2] * d[0] - o[0] * d[2];
    v[2] = o[0] * d[1] - o[1] * d[0];
    v[3] = d[0], v[4] = d[1], v[5] = d[2];
    const long long plane = (long long)H * W;
#pragma unroll
    for (int c = 0; c < 6; ++c)
        out[((long long)(c * 4 + j) * T + tt) * plane + (long long)y * W + x] = (bf16_t)f2bf(v[c]);
}

// one thread per (output row, channel c, dy): its 32 contiguous columns (dx, kh, kw) from four 8-pixel runs
__global__ __launch_bounds__(256) void camera_im2col_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out,
                                                            long long ldo, int C, int T, int H, int W,
                                                            long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int h16 = H >> 4, w16 = W >> 4;
    const int dy = (int)(i % 8);
    const int c = (int)((i / 8) % C);
    const long long row = i / (8LL * C);
    const int ox = (int)(row % w16);
    const int oy = (int)((row / w16) % h16);
    const int tt = (int)(row / ((long long)w16 * h16));
    const bf16_t* plane = in + ((long long)c * T + tt) * H * W;
    bf16_t px[4][8];                         // [kh 2 + kw][dx]
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int kw = 0; kw < 2; ++kw) {
            const u32x4_t v = *reinterpret_cast<const u32x4_t*>(plane + (long long)((2 * oy + kh) * 8 + dy) * W +
                                                                (2 * ox + kw) * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                px[kh * 2 + kw][2 * e] = (bf16_t)(v[e] & 0xffffu);
                px[kh * 2 + kw][2 * e + 1] = (bf16_t)(v[e] >> 16);
            }
        }
    bf16_t* dst = out + row * ldo + ((long long)c * 64 + dy * 8) * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {            // columns 8 q .. 8 q + 7: dx = 2 q, 2 q + 1
        u32x4_t o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int dx = 2 * q + (e >> 1), k0 = (e & 1) * 2;
            o[e] = (uint32_t)px[k0][dx] | ((uint32_t)px[k0 + 1][dx] << 16);
        }
        *reinterpret_cast<u32x4_t*>(dst + 8 * q) = o;
    }
}

__global__ __launch_bounds__(256) void relu_kernel(bf16_t* __restrict__ x, long long n8) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    u32x4_t v = reinterpret_cast<u32x4_t*>(x)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {            // a <= 0 ? +0 : a, as torch.relu on the device: -0 gives +0, a NaN stays
        const uint32_t lo = bflo(v[e]) <= 0.f ? 0u : (v[e] & 0xffffu);
        const uint32_t hi = bfhi(v[e]) <= 0.f ? 0u : (v[e] & 0xffff0000u);
        v[e] = lo | hi;
    }
    reinterpret_cast<u32x4_t*>(x)[i] = v;
}

}  // namespace

extern "C" int vs_ref_rows(const void* src, long long src_bs, void* dst, long long ldd, int batch, int n, int s,
                           int dim, void* stream) {
    if (!src || !dst || batch <= 0 || n <= 0 || s < 0 || dim <= 0 || dim % 8) return VS_E_INVALID;
    if (ldd < dim || (ldd & 7) || !al16(src) || !al16(dst)) return VS_E_INVALID;
    if (src_bs != 0 && (src_bs < (long long)n * dim || (src_bs & 7))) return VS_E_INVALID;
    const long long total = (long long)batch * n * (dim / 8);
    if (nblk256(total) == 0) return VS_E_INVALID;
    hipLaunchKernelGGL(ref_rows_kernel, dim3(nblk256(total)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src,
                       src_bs, (bf16_t*)dst, ldd, n, s, dim / 8, total);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_unpatchify_skip(const void* tokens, void* lat, int batch, int channels, int frames, int height,
                                  int width, int skip, void* stream) {
    if (!lat || !tokens || batch <= 0 || channels <= 0 || frames <= 0 || height <= 0 || width <= 0 || skip < 0)
        return VS_E_INVALID;
    if (height % 2 || width % 2 || (reinterpret_cast<uintptr_t>(lat) & 3) || (reinterpret_cast<uintptr_t>(tokens) & 1))
        return VS_E_INVALID;
    const long long total = (long long)batch * channels * frames * (height / 2) * (width / 2);
    if (nblk256(total) == 0) return VS_E_INVALID;
    hipLaunchKernelGGL(unpatchify_skip_kernel, dim3(nblk256(total)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)tokens, (bf16_t*)lat, channels, frames, height, width, (long long)skip, total);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_camera_rays(const float* intrinsics, const float* c2w, void* out, int frames, int t, int height,
                              int width, void* stream) {
    if (!intrinsics || !c2w || !out || frames <= 0 || t <= 0 || height <= 0 || width <= 0) return VS_E_INVALID;
    if ((long long)frames < 4LL * t - 3) return VS_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(intrinsics) & 3) || (reinterpret_cast<uintptr_t>(c2w) & 3) ||
        (reinterpret_cast<uintptr_t>(out) & 1))
        return VS_E_INVALID;
    const long long total = 4LL * t * height * width;
    if (nblk256(total) == 0) return VS_E_INVALID;
    hipLaunchKernelGGL(camera_rays_kernel, dim3(nblk256(total)), dim3(256), 0, (hipStream_t)stream, intrinsics, c2w,
                       (bf16_t*)out, t, height, width, total);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_camera_im2col(const void* in, void* out, long long ldo, int channels, int t, int height, int width,
                                void* stream) {
    if (!in || !out || channels <= 0 || t <= 0 || height <= 0 || width <= 0 || height % 16 || width % 16)
        return VS_E_INVALID;
    if (ldo < 256LL * channels || (ldo & 7) || !al16(in) || !al16(out)) return VS_E_INVALID;
    const long long total = (long long)t * (height / 16) * (width / 16) * channels * 8;
    if (nblk256(total) == 0) return VS_E_INVALID;
    hipLaunchKernelGGL(camera_im2col_kernel, dim3(nblk256(total)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)in,
                       (bf16_t*)out, ldo, channels, t, height, width, total);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_relu(void* x, long long n, void* stream) {
    if (!x || n <= 0 || n % 8 || !al16(x)) return VS_E_INVALID;
    if (nblk256(n / 8) == 0) return VS_E_INVALID;
    hipLaunchKernelGGL(relu_kernel, dim3(nblk256(n / 8)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)x, n / 8);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
