// The Wan2.2 VAE's own kernels (include/vstyler_vae22.h): the channel RMS norm at rows up to 1024 wide,
// the parameter-free shortcuts of Down_ResidualBlock / Up_ResidualBlock (AvgDown3D / DupUp3D) added in
// place onto the main path's output, the 2x2 pixel patchify and its inverse, and the attention softmax that
// keeps its probabilities as a bf16 hi / lo pair.  Row and elementwise
// kernels: one thread per 16-byte chunk of an output row (one wave per row for the norm), plain vector
// loads and stores, 64-bit indices, bounds from `total` alone.  The convolutions stay vs_vae_conv (vae.hip).
#include "common.h"
#include "../../include/vstyler_vae22.h"

namespace {

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
// blocks of 256 threads for `total` items, 0 when that does not fit a launch
inline unsigned nblk256(long long total) {
    const long long b = (total + 255) / 256;
    return b > 0x7fffffffLL ? 0u : (unsigned)b;
}

// Channel RMS norm (+SiLU), vae_rmsnorm_kernel's arithmetic at c <= 1024: one wave per pixel, lane q owns
// the 16-B chunks q and q + 64, so one load / store instruction moves 1 KB of one row (the whole row at
// c <= 512) and the row -- 2 KB at c = 1024 -- is read once and stays in registers (8 VGPRs of the 26 the
// kernel uses, no scratch, 8 waves per SIMD: -Rpass-analysis=kernel-resource-usage) between the norm and the write.  With
// the 16 lanes per pixel of the narrow kernel a lane would hold 8 chunks at c = 1024 and one instruction
// would take 256-B pieces of four rows 2 KB apart.
__global__ __launch_bounds__(256) void vae22_rmsnorm_kernel(const bf16_t* __restrict__ x, long long ldx,
                                                            bf16_t* __restrict__ y, long long ldy,
                                                            const bf16_t* __restrict__ gamma, long long npix,
                                                            int c, int silu, float scale) {
    constexpr int MAXN = 2;
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long pix = gid >> 6;           // wave-uniform
    const int q = (int)(gid & 63);
    if (pix >= npix) return;
    const int nck = c >> 3;                   // 16-B chunks per pixel
    const bf16_t* xr = x + pix * ldx;
    u32x4_t w[MAXN];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < MAXN; ++i) {
        const int k = q + 64 * i;
        if (k < nck) {
            w[i] = *(const u32x4_t*)(xr + k * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float a = bflo(w[i][e]), b = bfhi(w[i][e]);
                ss += a * a + b * b;
            }
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) ss += __shfl_xor(ss, o);
    const float nrm = fmaxf(rbf(sqrtf(ss)), 1e-12f);  // F.normalize: x / max(||x||, eps), norm in bf16
    const float rn = 1.0f / nrm;
    bf16_t* yr = y + pix * ldy;
#pragma unroll
    for (int i = 0; i < MAXN; ++i) {
        const int k = q + 64 * i;
        if (k >= nck) continue;
        const u32x4_t gw = *(const u32x4_t*)(gamma + k * 8);
        u32x4_t o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v0 = rbf(rbf(rbf(bflo(w[i][e]) * rn) * scale) * bflo(gw[e]));
            float v1 = rbf(rbf(rbf(bfhi(w[i][e]) * rn) * scale) * bfhi(gw[e]));
            if (silu) {
                v0 = v0 * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * v0));
                v1 = v1 * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * v1));
            }
            o[e] = pack2(v0, v1);
        }
        *(u32x4_t*)(yr + k * 8) = o;
    }
}

// one thread per 8 output channels of one output pixel: g input values per channel (input channel and
// (it, ih, iw) offset from the flat index o g + i), summed in fp32 in index order
__global__ __launch_bounds__(256) void vae22_avgdown_add_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
                                                                int t_in, int h_in, int w_in, int c_in, int c_out,
                                                                int ft, int fs, int t_out, int g, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int nch = c_out >> 3, ho = h_in / fs, wo = w_in / fs, fss = fs * fs, F = ft * fss;
    const int ch = (int)(i % nch);
    long long p = i / nch;                    // (b, j, yo, xo)
    const int xo = (int)(p % wo);
    p /= wo;
    const int yo = (int)(p % ho);
    p /= ho;
    const int j = (int)(p % t_out);
    const long long b = p / t_out;
    const float gf = (float)g;
    u32x4_t v = *reinterpret_cast<const u32x4_t*>(y + i * 8);
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int f0 = (ch * 8 + e) * g;
        float s = 0.f;
        for (int k = 0; k < g; ++k) {
            const int f = f0 + k;
            const int ci = f / F, r = f % F;
            const int it = r / fss, ih = (r / fs) % fs, iw = r % fs;
            const int tin = ft == 2 ? 2 * j - 1 + it : j;
            if (tin >= 0)
                s += bf2f(x[(((b * t_in + tin) * h_in + (yo * fs + ih)) * w_in + (xo * fs + iw)) * c_in + ci]);
        }
        acc[e] = rbf(s / gf);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = pack2(bflo(v[e]) + acc[2 * e], bfhi(v[e]) + acc[2 * e + 1]);
    *reinterpret_cast<u32x4_t*>(y + i * 8) = v;
}

// one thread per 8 output channels of one output pixel: each takes one input value
__global__ __launch_bounds__(256) void vae22_dupup_add_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
                                                              int t_in, int h_in, int w_in, int c_in, int c_out,
                                                              int ft, int fs, int t_out, int rep, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int nch = c_out >> 3, ho = h_in * fs, wo = w_in * fs, F = ft * fs * fs;
    const int ch = (int)(i % nch);
    long long p = i / nch;                    // (b, tau, yy, xx)
    const int xx = (int)(p % wo);
    p /= wo;
    const int yy = (int)(p % ho);
    p /= ho;
    const int tau = (int)(p % t_out);
    const long long b = p / t_out;
    const int tin = (tau + ft - 1) / ft, it = (tau + ft - 1) % ft;
    const int pos = it * fs * fs + (yy % fs) * fs + xx % fs;
    const bf16_t* xr = x + (((b * t_in + tin) * h_in + yy / fs) * w_in + xx / fs) * c_in;
    u32x4_t v = *reinterpret_cast<const u32x4_t*>(y + i * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int o = ch * 8 + 2 * e;
        v[e] = pack2(bflo(v[e]) + bf2f(xr[(o * F + pos) / rep]), bfhi(v[e]) + bf2f(xr[((o + 1) * F + pos) / rep]));
    }
    *reinterpret_cast<u32x4_t*>(y + i * 8) = v;
}

// one thread per output pixel: the RGB of its four source pixels (8-byte loads), 64 bytes out
__global__ __launch_bounds__(256) void vae22_patchify_kernel(const bf16_t* __restrict__ src, long long ld,
                                                             bf16_t* __restrict__ dst, int h, int w, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int h2 = h >> 1, w2 = w >> 1;
    const int xo = (int)(i % w2);
    const int yo = (int)((i / w2) % h2);
    const long long f = i / ((long long)w2 * h2);
    uint32_t px[2][2][3];                     // [q][r][c]
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const u32x2_t v = *reinterpret_cast<const u32x2_t*>(src + ((f * h + 2 * yo + q) * w + 2 * xo + r) * ld);
            px[q][r][0] = v[0] & 0xffffu, px[q][r][1] = v[0] >> 16, px[q][r][2] = v[1] & 0xffffu;
        }
    u32x4_t* d = reinterpret_cast<u32x4_t*>(dst + i * 32);
    u32x4_t o0, o1;
    const u32x4_t z = {0u, 0u, 0u, 0u};
    // channel 4 c + 2 r + q: pairs (r 0: q 0, q 1), (r 1: q 0, q 1) per colour
    o0[0] = px[0][0][0] | (px[1][0][0] << 16), o0[1] = px[0][1][0] | (px[1][1][0] << 16);
    o0[2] = px[0][0][1] | (px[1][0][1] << 16), o0[3] = px[0][1][1] | (px[1][1][1] << 16);
    o1[0] = px[0][0][2] | (px[1][0][2] << 16), o1[1] = px[0][1][2] | (px[1][1][2] << 16);
    o1[2] = 0u, o1[3] = 0u;
    d[0] = o0, d[1] = o1, d[2] = z, d[3] = z;
}

// one thread per source pixel: its 12 channels (8-byte loads), two 16-byte rows of two RGB0 pixels out
__global__ __launch_bounds__(256) void vae22_unpatchify_kernel(const bf16_t* __restrict__ src, long long ld,
                                                               bf16_t* __restrict__ dst, int h, int w,
                                                               long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int xi = (int)(i % w);
    const int yi = (int)((i / w) % h);
    const long long f = i / ((long long)w * h);
    uint32_t ch[12];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const u32x2_t v = *reinterpret_cast<const u32x2_t*>(src + i * ld + 4 * k);
        ch[4 * k] = v[0] & 0xffffu, ch[4 * k + 1] = v[0] >> 16, ch[4 * k + 2] = v[1] & 0xffffu, ch[4 * k + 3] = v[1] >> 16;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {             // row 2 yi + q: pixels r = 0, 1, each (R, G, B, 0)
        u32x4_t o;
        o[0] = ch[q] | (ch[4 + q] << 16), o[1] = ch[8 + q];
        o[2] = ch[2 + q] | (ch[6 + q] << 16), o[3] = ch[10 + q];
        *reinterpret_cast<u32x4_t*>(dst + ((f * 2 * h + 2 * yi + q) * (2LL * w) + 2 * xi) * 4) = o;
    }
}

// Attention softmax with the probabilities kept to ~16 bits: one wave per row of fp32 scores (vae_softmax_kernel's
// arithmetic: max, expf, one reciprocal), each p written as the bf16 pair hi = bf16(p), lo = bf16(p - hi) -- the
// difference is exact in fp32 -- at columns j and half + j, so that one bf16 GEMM over K = 2 half against V^T
// laid out twice sums hi V + lo V in fp32.  Pad columns of both halves are written as zero.
__global__ __launch_bounds__(256) void vae22_softmax_split_kernel(const float* __restrict__ s, long long ld_s,
                                                                  bf16_t* __restrict__ p, long long ld_p,
                                                                  long long rows, int ncols) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* sr = s + row * ld_s;
    bf16_t* pr = p + row * ld_p;
    const int half = (int)(ld_p >> 1);
    float mx = -INFINITY;
    for (int j = lane; j < ncols; j += 64) mx = fmaxf(mx, sr[j]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float sum = 0.f;
    for (int j = lane; j < ncols; j += 64) sum += expf(sr[j] - mx);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
    const float inv = 1.0f / sum;
    for (int j = lane; j < half; j += 64) {
        uint32_t hi = 0, lo = 0;
        if (j < ncols) {
            const float v = expf(sr[j] - mx) * inv;
            hi = f2bf(v);
            lo = f2bf(v - bf2f(hi));
        }
        pr[j] = (bf16_t)hi;
        pr[half + j] = (bf16_t)lo;
    }
}

// the shared argument rules of the two shortcuts; F and the other factor's divisibility
inline bool shortcut_args_ok(const void* x, const void* y, int n, int t_in, int h_in, int w_in, int c_in, int c_out,
                             int ft, int fs) {
    if (!x || !y || n <= 0 || t_in <= 0 || h_in <= 0 || w_in <= 0 || c_in <= 0 || c_out <= 0) return false;
    if ((ft != 1 && ft != 2) || (fs != 1 && fs != 2) || c_in % 8 || c_out % 8) return false;
    return al16(x) && al16(y);
}

}  // namespace

extern "C" int vs_vae22_rmsnorm(const void* x, long long ldx, void* y, long long ldy, const void* gamma,
                                long long npix, int c, int silu, void* stream) {
    if (!x || !y || !gamma || c <= 0 || c % 32 || c > 1024 || ldx < c || ldy < c || ldx % 8 || ldy % 8 || npix < 0)
        return VS_E_INVALID;
    if (!al16(x) || !al16(y) || !al16(gamma)) return VS_E_INVALID;
    if (npix == 0) return VS_OK;
    if (npix > (0x7fffffffLL << 2)) return VS_E_INVALID;
    hipLaunchKernelGGL(vae22_rmsnorm_kernel, dim3((unsigned)((npix + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)x, ldx, (bf16_t*)y, ldy, (const bf16_t*)gamma, npix, c, silu,
                       (float)sqrt((double)c));
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_vae22_avgdown_add(const void* x, void* y, int n, int t_in, int h_in, int w_in, int c_in, int c_out,
                                    int ft, int fs, void* stream) {
    if (!shortcut_args_ok(x, y, n, t_in, h_in, w_in, c_in, c_out, ft, fs)) return VS_E_INVALID;
    const long long cf = (long long)c_in * ft * fs * fs;
    if (cf % c_out || (ft == 2 && t_in % 2 == 0) || h_in % fs || w_in % fs) return VS_E_INVALID;
    const int t_out = ft == 2 ? 1 + (t_in - 1) / 2 : t_in;
    const long long total = (long long)n * t_out * (h_in / fs) * (w_in / fs) * (c_out / 8);
    if (nblk256(total) == 0) return VS_E_INVALID;
    hipLaunchKernelGGL(vae22_avgdown_add_kernel, dim3(nblk256(total)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)x, (bf16_t*)y, t_in, h_in, w_in, c_in, c_out, ft, fs, t_out, (int)(cf / c_out),
                       total);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_vae22_dupup_add(const void* x, void* y, int n, int t_in, int h_in, int w_in, int c_in, int c_out,
                                  int ft, int fs, void* stream) {
    if (!shortcut_args_ok(x, y, n, t_in, h_in, w_in, c_in, c_out, ft, fs)) return VS_E_INVALID;
    const long long cf = (long long)c_out * ft * fs * fs;
    if (cf % c_in) return VS_E_INVALID;
    const int t_out = ft * (t_in - 1) + 1;
    const long long total = (long long)n * t_out * ((long long)h_in * fs) * ((long long)w_in * fs) * (c_out / 8);
    if (nblk256(total) == 0) return VS_E_INVALID;
    hipLaunchKernelGGL(vae22_dupup_add_kernel, dim3(nblk256(total)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)x, (bf16_t*)y, t_in, h_in, w_in, c_in, c_out, ft, fs, t_out, (int)(cf / c_in),
                       total);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_vae22_patchify(const void* src, long long ld_src, void* dst, int nt, int h, int w, void* stream) {
    if (!src || !dst || nt <= 0 || h <= 0 || w <= 0 || h % 2 || w % 2 || ld_src < 4 || ld_src % 4) return VS_E_INVALID;
    if (!al8(src) || !al16(dst)) return VS_E_INVALID;
    const long long total = (long long)nt * (h / 2) * (w / 2);
    if (nblk256(total) == 0) return VS_E_INVALID;
    hipLaunchKernelGGL(vae22_patchify_kernel, dim3(nblk256(total)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)src, ld_src, (bf16_t*)dst, h, w, total);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_vae22_unpatchify(const void* src, long long ld_src, void* dst, int nt, int h, int w, void* stream) {
    if (!src || !dst || nt <= 0 || h <= 0 || w <= 0 || ld_src < 12 || ld_src % 4) return VS_E_INVALID;
    if (!al8(src) || !al16(dst)) return VS_E_INVALID;
    const long long total = (long long)nt * h * w;
    if (nblk256(total) == 0) return VS_E_INVALID;
    hipLaunchKernelGGL(vae22_unpatchify_kernel, dim3(nblk256(total)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)src, ld_src, (bf16_t*)dst, h, w, total);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_vae22_softmax_split(const float* s, long long ld_s, void* p, long long ld_p, long long rows,
                                      int ncols, void* stream) {
    if (!s || !p || ncols <= 0 || ld_s < ncols || ld_p % 2 || ld_p / 2 < ncols || ld_p > 0x7ffffffeLL || rows < 0)
        return VS_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(s) & 3) || (reinterpret_cast<uintptr_t>(p) & 1)) return VS_E_INVALID;
    if (rows == 0) return VS_OK;
    if (rows > (0x7fffffffLL << 2)) return VS_E_INVALID;
    hipLaunchKernelGGL(vae22_softmax_split_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       s, ld_s, (bf16_t*)p, ld_p, rows, ncols);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
