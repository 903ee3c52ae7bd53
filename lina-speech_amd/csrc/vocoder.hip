// vocoder.hip -- the two streaming kernels of the codes -> waveform step that follows the generation path
// (reference 3rdparty/decoder/modules.py:44-55, spectral_ops.py:36-75).  Channels-last
// activations [B, L, C] throughout (the reference transposes between [B,C,L] convolutions and [B,L,C] norms).
//
// K8  dwconv7 + LayerNorm: y[b,t,:] = LN_C( bias + sum_{j<7} w[:,j] * x[b, t-3+j, :] ) * scale[b or 0] + shift
//     -- ConvNeXtBlock.dwconv ("same" zero padding) fused with the LayerNorm / AdaLayerNorm that follows it
//     (modules.py:44-50, 62-82).  One wave per run of 8 consecutive rows of one b, lanes along the contiguous
//     channel dimension, a 7-row sliding window in registers (each x row is loaded once per wave), mean/variance
//     by wave shuffles.  HBM-bound streaming: (1 read + 1 write) * C * e bytes per row.
// K9  ISTFT overlap-add with "same" padding: every output sample gathers its <= ceil(win/hop) overlapping
//     windowed frames and divides by the window envelope (spectral_ops.py:56-75: two torch `fold`s and a
//     divide) -- no atomics, one pass, one thread per sample.
//
// Ragged batches (right-padded rows of different lengths, lens int32 [B] on the device): row b of a launch
// is, bit for bit, what the same entry gives for that row's own positions alone.
// K8r  K8 with a length per row: taps outside [0, L_b) read as zero, rows t >= L_b are written as zeros; a wave whose run lies
//      past L_b loads nothing.  The rows of a run go through K8's own body (dwconv7_ln_rows).
// K9r  K9 with T_b frames per row: sample n < T_b * hop gathers frames t <= T_b - 1 only, the rest of the row is zero.
// K10g GroupNorm over a row's own positions on channels-first data [B, C, Lmax] (the layout of backbone.pos_net), one
//      workgroup per (b, group): mean, then the centred sum of squares, then the affine result (optionally SiLU) for t < L_b
//      and zeros for t >= L_b.  The summation order is a function of the logical index (c - c0) * L_b + t alone.
#include <lina_dev.h>
#include "lina_common.h"

namespace lina {

constexpr int kDwMaxPer = 16;   // channels per lane: C <= 1024

constexpr int kDwRows = 8;      // consecutive time steps per wave: every x row is loaded once per wave (7 -> 1.75 reads/row)

// Rows [t0, t1) of ONE batch element whose live length is Lb (taps outside [0, Lb) read as zero): xb / yb its [*, C] rows,
// b its index into the scale / shift rows.  Called by a whole wave; K8 and K8r share it, so a row's arithmetic and its order
// are the same in both.
template <typename T, int PER>     // PER = channel groups of 64 per lane (C <= 64 * PER)
__device__ __forceinline__ void dwconv7_ln_rows(const T* __restrict__ xb, const T* __restrict__ w,
                                                const T* __restrict__ bias, const T* __restrict__ scale,
                                                const T* __restrict__ shift, T* __restrict__ yb, int b, int t0, int t1,
                                                int Lb, int C, int64_t scale_sb, float eps) {
    const int lane = threadIdx.x & 63;
    // sliding window win[j][i] = x[t - 3 + j][lane + 64 i], taps and the affine rows stay in registers
    float win[7][PER], wv[7][PER], bv[PER], sc[PER], sh[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int c = lane + 64 * i;
        const bool ok = c < C;
        bv[i] = (ok && bias) ? ld(bias + c) : 0.0f;
        sc[i] = (ok && scale) ? ld(scale + b * scale_sb + c) : 1.0f;
        sh[i] = (ok && shift) ? ld(shift + b * scale_sb + c) : 0.0f;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            wv[j][i] = ok ? ld(w + (int64_t)c * 7 + j) : 0.0f;
            const int tt = t0 - 4 + j;                        // one step behind: the loop shifts before it uses
            win[j][i] = (ok && j > 0 && tt >= 0 && tt < Lb) ? ld(xb + (int64_t)tt * C + c) : 0.0f;
        }
    }
    for (int t = t0; t < t1; ++t) {
        float z[PER];
        float s1 = 0.0f;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int c = lane + 64 * i;
            const bool ok = c < C;
#pragma unroll
            for (int j = 0; j < 6; ++j) win[j][i] = win[j + 1][i];
            win[6][i] = (ok && t + 3 < Lb) ? ld(xb + (int64_t)(t + 3) * C + c) : 0.0f;
            float acc = bv[i];
#pragma unroll
            for (int j = 0; j < 7; ++j) acc = fmaf(wv[j][i], win[j][i], acc);
            z[i] = ok ? acc : 0.0f;
            s1 += z[i];
        }
        s1 += shfl_xor(s1, 1); s1 += shfl_xor(s1, 2); s1 += shfl_xor(s1, 4);
        s1 += shfl_xor(s1, 8); s1 += shfl_xor(s1, 16); s1 += shfl_xor(s1, 32);
        const float mu = s1 / (float)C;
        float s2 = 0.0f;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int c = lane + 64 * i;
            if (c < C) { const float d = z[i] - mu; s2 += d * d; }
        }
        s2 += shfl_xor(s2, 1); s2 += shfl_xor(s2, 2); s2 += shfl_xor(s2, 4);
        s2 += shfl_xor(s2, 8); s2 += shfl_xor(s2, 16); s2 += shfl_xor(s2, 32);
        const float rstd = rsqrtf(s2 / (float)C + eps);
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int c = lane + 64 * i;
            if (c < C) st(yb + (int64_t)t * C + c, (z[i] - mu) * rstd * sc[i] + sh[i]);
        }
    }
}

template <typename T, int PER>
__global__ __launch_bounds__(256) void dwconv7_ln_kernel(const T* __restrict__ x, const T* __restrict__ w,
                                                         const T* __restrict__ bias, const T* __restrict__ scale,
                                                         const T* __restrict__ shift, T* __restrict__ y, int B, int L,
                                                         int C, int64_t scale_sb, float eps) {
    const int nblk = (L + kDwRows - 1) / kDwRows;             // row blocks per batch element
    const int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blk >= (int64_t)B * nblk) return;                     // whole wave
    const int b = (int)(blk / nblk);
    const int t0 = (int)(blk % nblk) * kDwRows;
    dwconv7_ln_rows<T, PER>(x + (int64_t)b * L * C, w, bias, scale, shift, y + (int64_t)b * L * C, b, t0,
                            min(t0 + kDwRows, L), L, C, scale_sb, eps);
}

// K8r: row b has lens[b] live time steps (clamped to [0, L]; L stays the row stride).  The run decomposition of a row is K8's
// (runs of 8 from t = 0), so the live rows are the instructions of K8 on x[b, :L_b] alone.
template <typename T, int PER>
__global__ __launch_bounds__(256) void dwconv7_ln_ragged_kernel(const T* __restrict__ x, const T* __restrict__ w,
                                                                const T* __restrict__ bias, const T* __restrict__ scale,
                                                                const T* __restrict__ shift, T* __restrict__ y,
                                                                const int32_t* __restrict__ lens, int B, int L, int C,
                                                                int64_t scale_sb, float eps) {
    const int lane = threadIdx.x & 63;
    const int nblk = (L + kDwRows - 1) / kDwRows;
    const int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blk >= (int64_t)B * nblk) return;                     // whole wave
    const int b = (int)(blk / nblk);
    const int t0 = (int)(blk % nblk) * kDwRows;
    const int Lb = min(max((int)lens[b], 0), L);
    const int t_end = min(t0 + kDwRows, L);
    const int t1 = min(t_end, Lb);                            // live rows of this run: [t0, t1)
    T* yb = y + (int64_t)b * L * C;
    if (t1 > t0)
        dwconv7_ln_rows<T, PER>(x + (int64_t)b * L * C, w, bias, scale, shift, yb, b, t0, t1, Lb, C, scale_sb, eps);
    for (int t = max(t0, t1); t < t_end; ++t) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int c = lane + 64 * i;
            if (c < C) st(yb + (int64_t)t * C + c, 0.0f);
        }
    }
}

// One output sample of a row of T frames: fb the row's frames [T, win] (inverse-transformed, NOT yet windowed), p the position
// in the un-trimmed overlap-add buffer.  K9 and K9r share it.
__device__ __forceinline__ float istft_ola_sample(const float* __restrict__ fb, const float* __restrict__ window, int T,
                                                  int win, int hop, int p) {
    int t_hi = p / hop;
    if (t_hi > T - 1) t_hi = T - 1;
    float acc = 0.0f, env = 0.0f;
    for (int t = t_hi; t >= 0; --t) {
        const int k = p - t * hop;
        if (k >= win) break;
        const float wv = window[k];
        acc = fmaf(fb[(int64_t)t * win + k], wv, acc);
        env = fmaf(wv, wv, env);
    }
    return acc / env;
}

// frames [B, T, win] (already inverse-transformed, NOT yet windowed), window [win] fp32, y [B, n_out] fp32,
// n_out = (T-1)*hop + win - 2*pad
__global__ __launch_bounds__(256) void istft_ola_kernel(const float* __restrict__ frames, const float* __restrict__ window,
                                                        float* __restrict__ y, int T, int win, int hop, int pad,
                                                        int n_out) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (n >= n_out) return;
    y[(int64_t)b * n_out + n] = istft_ola_sample(frames + (int64_t)b * T * win, window, T, win, hop, n + pad);
}

// K9r: row b holds lens[b] frames (clamped to [0, T]; T stays the row stride), win - hop even: y [B, T*hop], row b's first
// T_b * hop samples are K9's on frames[b, :T_b] alone, the rest zeros.
__global__ __launch_bounds__(256) void istft_ola_ragged_kernel(const float* __restrict__ frames,
                                                               const float* __restrict__ window, float* __restrict__ y,
                                                               const int32_t* __restrict__ lens, int T, int win, int hop,
                                                               int pad, int n_out) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (n >= n_out) return;
    const int Tb = min(max((int)lens[b], 0), T);
    y[(int64_t)b * n_out + n] =
        n < Tb * hop ? istft_ola_sample(frames + (int64_t)b * T * win, window, Tb, win, hop, n + pad) : 0.0f;
}

// K10g: one workgroup of 256 threads per (b, group).  The group's live elements are numbered i = (c - c0) * Lb + t; thread tid
// owns i = tid + 256 j (j = 0, 1, ...) and adds them into four partial sums by j % 4, in the order of j; the four are added as
// (s0 + s1) + (s2 + s3), the 64 lanes of a wave by a butterfly, the four waves through LDS as (w0 + w1) + (w2 + w3).  None
// of this depends on Lmax, the row stride or b: a row is bit-equal to itself alone.
constexpr int kGnThreads = 256;

template <class F>
__device__ __forceinline__ void gn_walk(int N, int Lb, F f) {           // f(k, c - c0, t) for the thread's elements
    const int tid = threadIdx.x;
    const int qs = kGnThreads / Lb, rs = kGnThreads % Lb;
    int c = tid / Lb, t = tid % Lb;
    for (int i = tid; i < N; i += 4 * kGnThreads) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i + k * kGnThreads < N) f(k, c, t);
            c += qs;
            t += rs;
            if (t >= Lb) { t -= Lb; ++c; }
        }
    }
}

__device__ __forceinline__ float gn_block_sum(const float (&acc)[4], float* red) {      // red: 4 floats of LDS, used once
    float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    s += shfl_xor(s, 1); s += shfl_xor(s, 2); s += shfl_xor(s, 4);
    s += shfl_xor(s, 8); s += shfl_xor(s, 16); s += shfl_xor(s, 32);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

template <typename T>
__global__ __launch_bounds__(kGnThreads) void group_norm_ragged_kernel(const T* __restrict__ x, const T* __restrict__ weight,
                                                                       const T* __restrict__ bias, T* __restrict__ y,
                                                                       const int32_t* __restrict__ lens, int C, int L, int G,
                                                                       float eps, int act) {
    __shared__ float red1[4], red2[4];
    const int b = blockIdx.x / G, g = blockIdx.x % G;
    const int Cg = C / G, c0 = g * Cg;
    const int Lb = lens ? min(max((int)lens[b], 0), L) : L;
    const T* xg = x + ((int64_t)b * C + c0) * L;
    T* yg = y + ((int64_t)b * C + c0) * L;
    const int N = Cg * Lb;
    if (N > 0) {                                                      // (block-uniform)
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        gn_walk(N, Lb, [&](int k, int c, int t) { acc[k] += ld(xg + (int64_t)c * L + t); });
        const float mean = gn_block_sum(acc, red1) / (float)N;
        float acc2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        gn_walk(N, Lb, [&](int k, int c, int t) {
            const float d = ld(xg + (int64_t)c * L + t) - mean;
            acc2[k] = fmaf(d, d, acc2[k]);
        });
        const float rstd = rsqrtf(gn_block_sum(acc2, red2) / (float)N + eps);
        gn_walk(N, Lb, [&](int k, int c, int t) {
            const float wc = weight ? ld(weight + c0 + c) : 1.0f, bc = bias ? ld(bias + c0 + c) : 0.0f;
            float v = (ld(xg + (int64_t)c * L + t) - mean) * rstd * wc + bc;
            if (act == LINA_ACT_SILU) v = silu(v);
            st(yg + (int64_t)c * L + t, v);
        });
    }
    const int tail = L - Lb;                                          // zeros for t >= Lb
    for (int i = threadIdx.x; i < Cg * tail; i += kGnThreads) st(yg + (int64_t)(i / tail) * L + Lb + i % tail, 0.0f);
}

}  // namespace lina

extern "C" int lina_dwconv7_ln(const void* x, const void* w, const void* bias, const void* scale, const void* shift,
                               void* y, int B, int L, int C, int64_t scale_sb, float eps, int dtype,
                               lina_stream_t stream) {
    using namespace lina;
    LINA_REQUIRE(x && w && y, "lina_dwconv7_ln: null pointer");
    LINA_REQUIRE(B > 0 && L > 0 && C > 0, "lina_dwconv7_ln: B,L,C must be positive (got %d,%d,%d)", B, L, C);
    LINA_REQUIRE(valid_dtype(dtype), "lina_dwconv7_ln: bad dtype %d", dtype);
    if (C > 64 * kDwMaxPer) return fail(LINA_ERR_UNSUPPORTED, "lina_dwconv7_ln: C=%d exceeds %d", C, 64 * kDwMaxPer);
    const int64_t blocks = (int64_t)B * ((L + kDwRows - 1) / kDwRows);
    dim3 grid((unsigned)((blocks + 3) / 4));
#define LINA_DW(TT, PP)                                                                                              \
    LINA_LAUNCH((dwconv7_ln_kernel<TT, PP>), grid, dim3(256), 0, stream, (const TT*)x, (const TT*)w, (const TT*)bias, \
                (const TT*)scale, (const TT*)shift, (TT*)y, B, L, C, scale_sb, eps)
#define LINA_DW_T(TT)                                                                          \
    do {                                                                                       \
        if (C <= 256) LINA_DW(TT, 4); else if (C <= 512) LINA_DW(TT, 8);                       \
        else if (C <= 768) LINA_DW(TT, 12); else LINA_DW(TT, 16);                              \
    } while (0)
    if (dtype == LINA_F32) LINA_DW_T(float); else LINA_DW_T(bf16_t);
#undef LINA_DW_T
#undef LINA_DW
    return check_launch("lina_dwconv7_ln");
}

extern "C" int lina_istft_ola(const float* frames, const float* window, float* y, int B, int T, int win, int hop,
                              lina_stream_t stream) {
    using namespace lina;
    LINA_REQUIRE(frames && window && y, "lina_istft_ola: null pointer");
    LINA_REQUIRE(B > 0 && T > 0 && win > 0 && hop > 0 && hop <= win, "lina_istft_ola: bad shape");
    const int pad = (win - hop) / 2;
    const int n_out = (T - 1) * hop + win - 2 * pad;
    LINA_REQUIRE(n_out > 0, "lina_istft_ola: empty output");
    dim3 grid((unsigned)((n_out + 255) / 256), (unsigned)B);
    LINA_LAUNCH(istft_ola_kernel, grid, dim3(256), 0, stream, frames, window, y, T, win, hop, pad, n_out);
    return check_launch("lina_istft_ola");
}

extern "C" int lina_dwconv7_ln_ragged(const void* x, const void* w, const void* bias, const void* scale,
                                      const void* shift, void* y, const int32_t* lens, int B, int L, int C,
                                      int64_t scale_sb, float eps, int dtype, lina_stream_t stream) {
    using namespace lina;
    LINA_REQUIRE(x && w && y && lens, "lina_dwconv7_ln_ragged: null pointer");
    LINA_REQUIRE(B > 0 && L > 0 && C > 0, "lina_dwconv7_ln_ragged: B,L,C must be positive (got %d,%d,%d)", B, L, C);
    LINA_REQUIRE(valid_dtype(dtype), "lina_dwconv7_ln_ragged: bad dtype %d", dtype);
    if (C > 64 * kDwMaxPer)
        return fail(LINA_ERR_UNSUPPORTED, "lina_dwconv7_ln_ragged: C=%d exceeds %d", C, 64 * kDwMaxPer);
    const int64_t blocks = (int64_t)B * ((L + kDwRows - 1) / kDwRows);
    dim3 grid((unsigned)((blocks + 3) / 4));
#define LINA_DW(TT, PP)                                                                                                \
    LINA_LAUNCH((dwconv7_ln_ragged_kernel<TT, PP>), grid, dim3(256), 0, stream, (const TT*)x, (const TT*)w,            \
                (const TT*)bias, (const TT*)scale, (const TT*)shift, (TT*)y, lens, B, L, C, scale_sb, eps)
#define LINA_DW_T(TT)                                                                          \
    do {                                                                                       \
        if (C <= 256) LINA_DW(TT, 4); else if (C <= 512) LINA_DW(TT, 8);                       \
        else if (C <= 768) LINA_DW(TT, 12); else LINA_DW(TT, 16);                              \
    } while (0)
    if (dtype == LINA_F32) LINA_DW_T(float); else LINA_DW_T(bf16_t);
#undef LINA_DW_T
#undef LINA_DW
    return check_launch("lina_dwconv7_ln_ragged");
}

extern "C" int lina_istft_ola_ragged(const float* frames, const float* window, float* y, const int32_t* lens, int B,
                                     int T, int win, int hop, lina_stream_t stream) {
    using namespace lina;
    LINA_REQUIRE(frames && window && y && lens, "lina_istft_ola_ragged: null pointer");
    LINA_REQUIRE(B > 0 && T > 0 && win > 0 && hop > 0 && hop <= win, "lina_istft_ola_ragged: bad shape");
    LINA_REQUIRE((win - hop) % 2 == 0, "lina_istft_ola_ragged: win - hop must be even (got %d, %d)", win, hop);
    LINA_REQUIRE((int64_t)T * hop < ((int64_t)1 << 31), "lina_istft_ola_ragged: T * hop exceeds 2^31");
    const int pad = (win - hop) / 2;
    const int n_out = T * hop;
    dim3 grid((unsigned)((n_out + 255) / 256), (unsigned)B);
    LINA_LAUNCH(istft_ola_ragged_kernel, grid, dim3(256), 0, stream, frames, window, y, lens, T, win, hop, pad, n_out);
    return check_launch("lina_istft_ola_ragged");
}

extern "C" int lina_group_norm_ragged(const void* x, const void* weight, const void* bias, void* y,
                                      const int32_t* lens, int B, int C, int L, int G, float eps, int act, int dtype,
                                      lina_stream_t stream) {
    using namespace lina;
    LINA_REQUIRE(x && y, "lina_group_norm_ragged: null pointer");
    LINA_REQUIRE(B > 0 && C > 0 && L > 0 && G > 0, "lina_group_norm_ragged: B,C,L,G must be positive (got %d,%d,%d,%d)", B,
                 C, L, G);
    LINA_REQUIRE(C % G == 0, "lina_group_norm_ragged: C=%d is not divisible by G=%d", C, G);
    LINA_REQUIRE(act == LINA_ACT_NONE || act == LINA_ACT_SILU, "lina_group_norm_ragged: bad act %d", act);
    LINA_REQUIRE(valid_dtype(dtype), "lina_group_norm_ragged: bad dtype %d", dtype);
    LINA_REQUIRE((int64_t)(C / G) * L < ((int64_t)1 << 30), "lina_group_norm_ragged: a group of %d x %d elements is too large",
                 C / G, L);
    LINA_REQUIRE((int64_t)B * G < ((int64_t)1 << 31), "lina_group_norm_ragged: B * G exceeds 2^31");
    dim3 grid((unsigned)(B * G));
    if (dtype == LINA_F32)
        LINA_LAUNCH(group_norm_ragged_kernel<float>, grid, dim3(kGnThreads), 0, stream, (const float*)x, (const float*)weight,
                    (const float*)bias, (float*)y, lens, C, L, G, eps, act);
    else
        LINA_LAUNCH(group_norm_ragged_kernel<bf16_t>, grid, dim3(kGnThreads), 0, stream, (const bf16_t*)x,
                    (const bf16_t*)weight, (const bf16_t*)bias, (bf16_t*)y, lens, C, L, G, eps, act);
    return check_launch("lina_group_norm_ragged");
}
