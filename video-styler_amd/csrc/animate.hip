// Wan2.2-Animate (include/vstyler_animate.h): the face adapter's per-frame cross-attention with the
// per-head RMSNorm of q fused in, that norm alone (K, once per call), and the face encoder's
// LayerNorm -> SiLU.
//
// vs_face_attn is a streaming VALU kernel: 5 keys per frame are no MFMA tile.  One head is 256 B =
// 16 lanes x 16 B, so a wave covers 4 heads of one token row per load and every reduction over a head is a
// 16-lane DPP tree.  A wave keeps the K and V chunks of its 4 heads and its frame in registers (fp32,
// 16 floats per key) and walks that frame's tokens, so K / V are read once per (frame, token chunk, head
// group) and each q / o element moves once.
#include "common.h"
#include "../../include/vstyler_animate.h"

namespace {

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

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

// the sum over the 16 lanes of a DPP row, the same bits in each of them: lane pairs, quads, then the
// mirrored half and the mirrored row (after the quad steps every lane of a quad holds the quad's sum, so
// a mirror pairs each half / row with its other one); every step adds two operands, in either order
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_f<0xB1>(v);     // quad_perm [1, 0, 3, 2]
    v += dpp_f<0x4E>(v);     // quad_perm [2, 3, 0, 1]
    v += dpp_f<0x141>(v);    // row_half_mirror
    v += dpp_f<0x140>(v);    // row_mirror
    return v;
}

// The per-head RMSNorm on one lane's 8 columns of a 128-wide head (its 16 lanes call together): the
// reference RMSNorm's two roundings.  vs_face_attn's qn and vs_head_rmsnorm are this one function.
__device__ __forceinline__ void head_rmsnorm8(const float* x, const float* w, float eps, float* y) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s += x[e] * x[e];
    s = row16_sum(s);
    const float r = rsqrtf(s * (1.0f / 128.0f) + eps);
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = rbf(rbf(x[e] * r) * w[e]);
}

constexpr int FA_CH = 128;      // tokens of one frame per block: 32 per wave against one K / V load

// Block = 4 waves on one (sample, frame, chunk of FA_CH tokens, group of 4 heads); wave w takes the
// chunk's tokens w, w + 4, ...  q and o are not __restrict__: o may be q (each lane reads its chunk
// before it writes it).
template <int NK>
__global__ __launch_bounds__(256) void face_attn_kernel(const bf16_t* q, long long ldq, const bf16_t* __restrict__ k,
                                                        const bf16_t* __restrict__ v, long long ldkv, long long kv_bs,
                                                        bf16_t* o, long long ldo, const bf16_t* __restrict__ wq,
                                                        int rpb, int heads, int frames, int tpf, int tok_off,
                                                        int ngroups, int nchunk, int nfl, float eps, float scale) {
    const int g = blockIdx.x % ngroups;
    long long item = blockIdx.x / ngroups;
    const int c = (int)(item % nchunk);
    item /= nchunk;
    const int f = tok_off / tpf + (int)(item % nfl);
    const long long b = item / nfl;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (g * 4 + (lane >> 4) >= heads) return;                 // whole 16-lane rows leave together
    const long long col = (long long)g * 512 + lane * 8;
    // this block's tokens of frame f that are rows of this call
    const long long fbase = (long long)f * tpf;
    const long long t0 = max(fbase + (long long)c * FA_CH, (long long)tok_off);
    const long long t1 = min(fbase + min((long long)(c + 1) * FA_CH, (long long)tpf), (long long)tok_off + rpb);
    if (t0 + wave >= t1) return;
    const long long rbase = b * rpb - tok_off;                // row of token t: rbase + t
    if (f >= frames) {                                        // pad rows
        const u32x4_t z = {0u, 0u, 0u, 0u};
        for (long long t = t0 + wave; t < t1; t += 4) *reinterpret_cast<u32x4_t*>(o + (rbase + t) * ldo + col) = z;
        return;
    }
    float kk[NK][8], vv[NK][8], w[8];
    {
        const long long kvrow = b * kv_bs + (long long)f * NK * ldkv + col;
#pragma unroll
        for (int j = 0; j < NK; ++j) {
            unpack8(*reinterpret_cast<const u32x4_t*>(k + kvrow + j * ldkv), kk[j]);
            unpack8(*reinterpret_cast<const u32x4_t*>(v + kvrow + j * ldkv), vv[j]);
        }
        unpack8(*reinterpret_cast<const u32x4_t*>(wq + (lane & 15) * 8), w);
    }
    long long t = t0 + wave;
    u32x4_t cur = *reinterpret_cast<const u32x4_t*>(q + (rbase + t) * ldq + col);
    for (; t < t1; t += 4) {
        u32x4_t nxt = cur;
        if (t + 4 < t1) nxt = *reinterpret_cast<const u32x4_t*>(q + (rbase + t + 4) * ldq + col);
        float x[8], qn[8], s[NK];
        unpack8(cur, x);
        head_rmsnorm8(x, w, eps, qn);
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < NK; ++j) {
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) d += qn[e] * kk[j][e];
            s[j] = scale * row16_sum(d);
            m = fmaxf(m, s[j]);
        }
        float l = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NK; ++j) {
            const float p = expf(s[j] - m);
            l += p;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += p * vv[j][e];
        }
        const float rl = 1.0f / l;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] *= rl;
        *reinterpret_cast<u32x4_t*>(o + (rbase + t) * ldo + col) = pack8(acc);
        cur = nxt;
    }
}

// one lane per 16-byte chunk of a head; 16 consecutive lanes are one head of one row
__global__ __launch_bounds__(256) void head_rmsnorm_kernel(bf16_t* __restrict__ x, long long ldx, int heads,
                                                           const bf16_t* __restrict__ w, float eps, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;                                   // total % 16 == 0: whole rows of 16 lanes
    const int per_row = heads * 16;
    const long long row = i / per_row;
    const int ch = (int)(i % per_row);
    bf16_t* p = x + row * ldx + ch * 8;
    float xv[8], wv[8], y[8];
    unpack8(*reinterpret_cast<const u32x4_t*>(p), xv);
    unpack8(*reinterpret_cast<const u32x4_t*>(w + (ch & 15) * 8), wv);
    head_rmsnorm8(xv, wv, eps, y);
    *reinterpret_cast<u32x4_t*>(p) = pack8(y);
}

constexpr int LS_T = 128;       // threads per row
constexpr int LS_MC = 8;        // 8-element chunks per thread: dim <= 8192

__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < LS_T / 64; ++i) t += red[i];
    return t;
}

// bf16 bits of a double, round-to-nearest-even in one step (as elementwise.hip's d2bf)
__device__ __forceinline__ uint32_t d2bf(double d) {
    const uint64_t u = __builtin_bit_cast(uint64_t, d);
    const uint32_t sign = (uint32_t)(u >> 48) & 0x8000u;
    const double a = fabs(d);
    if (!(a < INFINITY)) return a == INFINITY ? (sign | 0x7F80u) : 0x7FC0u;
    if (a < 0x1p-126) return sign | (uint32_t)rint(a * 0x1p133);
    const uint64_t m = u & 0x7FFFFFFFFFFFFFFFull;
    const uint64_t r = (m + ((1ull << 44) - 1) + ((m >> 45) & 1)) >> 45;
    const uint64_t v = r - ((uint64_t)(1023 - 127) << 7);
    return sign | (v >= 0x7F80u ? 0x7F80u : (uint32_t)v);
}
// silu in double: h / (1 + exp(-h)); exp(-h) = inf for h < -709.8 gives -0 (the limit)
__device__ __forceinline__ uint32_t silu_bf(float h) {
    const double d = (double)h;
    return d2bf(d / (1.0 + exp(-d)));
}

// one block per row: LayerNorm statistics as ln_modulate_kernel (elementwise.hip), the row in registers;
// a few hundred rows once per call, so SiLU is evaluated in double
__global__ __launch_bounds__(LS_T) void ln_silu_kernel(const bf16_t* x, long long ldx, bf16_t* out, long long ldo,
                                                       int dim, int norm, float eps) {
    __shared__ float red[LS_T / 64];
    const long long row = blockIdx.x;
    const int nch = dim >> 3;
    const bf16_t* xr = x + row * ldx;
    float v[LS_MC][8];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < LS_MC; ++c) {
        const int ch = threadIdx.x + c * LS_T;
        if (ch < nch) {
            unpack8(*reinterpret_cast<const u32x4_t*>(xr + ch * 8), v[c]);
#pragma unroll
            for (int e = 0; e < 8; ++e) s += v[c][e];
        }
    }
    float mean = 0.f, rstd = 1.f;
    if (norm) {                                               // uniform over the grid
        mean = block_sum(s, red) / dim;
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < LS_MC; ++c) {
            const int ch = threadIdx.x + c * LS_T;
            if (ch < nch) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = v[c][e] - mean;
                    q += d * d;
                }
            }
        }
        rstd = rsqrtf(block_sum(q, red) / dim + eps);
    }
    bf16_t* orow = out + row * ldo;
#pragma unroll
    for (int c = 0; c < LS_MC; ++c) {
        const int ch = threadIdx.x + c * LS_T;
        if (ch >= nch) continue;
        u32x4_t w;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float lo = norm ? rbf((v[c][2 * e] - mean) * rstd) : v[c][2 * e];
            const float hi = norm ? rbf((v[c][2 * e + 1] - mean) * rstd) : v[c][2 * e + 1];
            w[e] = silu_bf(lo) | (silu_bf(hi) << 16);
        }
        *reinterpret_cast<u32x4_t*>(orow + ch * 8) = w;
    }
}

// byte ranges [a, a + na) and [b, b + nb) share a byte
inline bool overlaps(const void* a, long long na, const void* b, long long nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

template <int NK>
void launch_face_attn(unsigned blocks, hipStream_t st, const bf16_t* q, long long ldq, const bf16_t* k,
                      const bf16_t* v, long long ldkv, long long kv_bs, bf16_t* o, long long ldo, const bf16_t* wq,
                      int rpb, int heads, int frames, int tpf, int tok_off, int ngroups, int nchunk, int nfl,
                      float eps, float scale) {
    hipLaunchKernelGGL(face_attn_kernel<NK>, dim3(blocks), dim3(256), 0, st, q, ldq, k, v, ldkv, kv_bs, o, ldo, wq,
                       rpb, heads, frames, tpf, tok_off, ngroups, nchunk, nfl, eps, scale);
}

}  // namespace

extern "C" int vs_face_attn(const void* q, long long ldq, const void* k, const void* v, long long ldkv,
                            long long kv_bs, void* o, long long ldo, const void* wq, int batch, int rows_per_batch,
                            int heads, int head_dim, int frames, int tokens_per_frame, int nkeys, int token_offset,
                            float eps, float scale, void* stream) {
    if (!q || !k || !v || !o || !wq || batch <= 0 || rows_per_batch <= 0 || heads <= 0 || head_dim <= 0 ||
        frames <= 0 || tokens_per_frame <= 0 || nkeys < 1 || nkeys > 8 || token_offset < 0)
        return VS_E_INVALID;
    if (!(eps >= 0.f) || !(scale - scale == 0.f)) return VS_E_INVALID;
    if (head_dim != 128) return VS_E_UNSUPPORTED;
    const long long width = 128LL * heads;
    if (ldq < width || ldo < width || ldkv < width || (ldq & 7) || (ldo & 7) || (ldkv & 7)) return VS_E_INVALID;
    const long long kv_extent = ((long long)frames * nkeys - 1) * ldkv + width;
    if (kv_bs != 0 && (kv_bs < kv_extent || (kv_bs & 7))) return VS_E_INVALID;
    if (!al16(q) || !al16(k) || !al16(v) || !al16(o) || !al16(wq)) return VS_E_INVALID;
    if ((long long)token_offset + rows_per_batch > 0x7fffffffLL) return VS_E_INVALID;
    const long long rows = (long long)batch * rows_per_batch;
    const long long q_bytes = ((rows - 1) * ldq + width) * 2, o_bytes = ((rows - 1) * ldo + width) * 2;
    const long long kv_bytes = ((kv_bs ? (batch - 1) * kv_bs : 0) + kv_extent) * 2;
    if (!(q == o && ldq == ldo) && overlaps(o, o_bytes, q, q_bytes)) return VS_E_INVALID;
    if (overlaps(o, o_bytes, k, kv_bytes) || overlaps(o, o_bytes, v, kv_bytes) || overlaps(o, o_bytes, wq, 256))
        return VS_E_INVALID;
    const int ngroups = (heads + 3) / 4;
    const int nchunk = (tokens_per_frame + FA_CH - 1) / FA_CH;
    const int nfl = (int)(((long long)token_offset + rows_per_batch - 1) / tokens_per_frame) -
                    token_offset / tokens_per_frame + 1;
    const long long blocks = (long long)batch * nfl * nchunk * ngroups;
    if (blocks > 0x7fffffffLL) return VS_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
#define VS_FA(N)                                                                                                   \
    case N:                                                                                                        \
        launch_face_attn<N>((unsigned)blocks, st, (const bf16_t*)q, ldq, (const bf16_t*)k, (const bf16_t*)v, ldkv, \
                            kv_bs, (bf16_t*)o, ldo, (const bf16_t*)wq, rows_per_batch, heads, frames,              \
                            tokens_per_frame, token_offset, ngroups, nchunk, nfl, eps, scale);                     \
        break;
    switch (nkeys) {
        VS_FA(1) VS_FA(2) VS_FA(3) VS_FA(4) VS_FA(5) VS_FA(6) VS_FA(7) VS_FA(8)
    }
#undef VS_FA
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_head_rmsnorm(void* x, long long ldx, int rows, int heads, int head_dim, const void* w, float eps,
                               void* stream) {
    if (!x || !w || rows <= 0 || heads <= 0 || head_dim <= 0 || !(eps >= 0.f)) return VS_E_INVALID;
    if (head_dim != 128) return VS_E_UNSUPPORTED;
    if (ldx < 128LL * heads || (ldx & 7) || !al16(x) || !al16(w)) return VS_E_INVALID;
    const long long total = (long long)rows * heads * 16;
    const long long blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return VS_E_INVALID;
    hipLaunchKernelGGL(head_rmsnorm_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (bf16_t*)x, ldx,
                       heads, (const bf16_t*)w, eps, total);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_ln_silu(const void* x, long long ldx, void* out, long long ldo, int rows, int dim, int norm,
                          float eps, void* stream) {
    if (!x || !out || rows <= 0 || dim <= 0 || dim % 8 || dim > LS_T * LS_MC * 8 || !(eps >= 0.f)) return VS_E_INVALID;
    if (ldx < dim || ldo < dim || (ldx & 7) || (ldo & 7) || !al16(x) || !al16(out)) return VS_E_INVALID;
    const long long x_bytes = (((long long)rows - 1) * ldx + dim) * 2, o_bytes = (((long long)rows - 1) * ldo + dim) * 2;
    if (!(x == out && ldx == ldo) && overlaps(out, o_bytes, x, x_bytes)) return VS_E_INVALID;
    hipLaunchKernelGGL(ln_silu_kernel, dim3((unsigned)rows), dim3(LS_T), 0, (hipStream_t)stream, (const bf16_t*)x, ldx,
                       (bf16_t*)out, ldo, dim, norm, eps);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
