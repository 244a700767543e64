// Row / glue kernels of the RAGGED passes (forward; backward of the speaker encoder: avc_backward_ragged; backward of the content encoder:
// avc_content_backward_ragged; backward of the decoder: avc_decoder_backward_ragged) (AE.inference over utterances of different lengths in one launch set;
// reference: inference.py:54-70, model.py:387-391 -- the reference converts one utterance per call).
//
// Packed buffers: sample b owns a contiguous [channels][T_b] block starting at element channels * off[b] (off = prefix sums
// of the per-sample lengths at that level).  InstanceNorm statistics, reflect padding and ceil-mode pooling all depend on the
// TRUE length of a sample, so nothing is padded: every row is processed at its own length.
#include <hip/hip_runtime.h>

#include "avc_common.h"
#include "avc_internal.h"

static __device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// nn.InstanceNorm1d(affine=False) (model.py:296,341) [+ append_cond, model.py:77-83] + ReLU [+ residual join]: one wavefront
// per row (b, c), three cached passes over the row's own T_b frames -- the arithmetic (two-pass statistics, in_xhat / in_preact)
// is instnorm_fwd_generic_kernel's of rowops.hip.
__global__ void __launch_bounds__(AVC_THREADS) rag_instnorm_fwd_kernel(const RagINArgs a) {
    const int tid = threadIdx.x, l = tid & 63;
    const int row = blockIdx.x * 4 + (tid >> 6);
    if (row >= a.B * a.C) return;   // (whole wavefronts leave together: a row is one wavefront)
    const int b = row / a.C, c = row - b * a.C;
    const int T = a.T[b];
    const long base = (long)a.C * a.off[b] + (long)c * T;
    const float* yrow = a.y + base;
    float s = 0.f;
    for (int t = l; t < T; t += 64) s += yrow[t];
    const float invT = 1.0f / (float)T;
    const float mean = wave_sum(s) / (float)T;   // see in_xhat
    float ss = 0.f;
    for (int t = l; t < T; t += 64) {
        float d = yrow[t] - mean;
        ss += d * d;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(ss) * invT + AVC_IN_EPS);   // biased variance
    float gamma = 1.f, beta = 0.f;
    if (a.cond) {
        const float* cr = a.cond + (long)b * a.cond_sb + a.cond_off;
        beta = cr[c];
        gamma = cr[a.C + c];
    }
    if (a.mean && l == 0) {   // (plans with a backward pass: the statistics it normalises by, so that its ReLU decision is this pass's)
        a.mean[row] = mean;
        a.rstd[row] = rstd;
    }
    float* orow = a.out + base;
    int Tres = 0;
    const float* rrow = nullptr;
    if (a.res) {
        Tres = a.Tres[b];
        rrow = a.res + (long)a.C * a.offres[b] + (long)c * Tres;
    }
    for (int t = l; t < T; t += 64) {
        float w = avc_act(in_preact(in_xhat(yrow[t], mean, rstd), gamma, beta), a.slope);
        if (rrow) {
            if (a.res_mode == AVC_RES_IDENTITY)
                w += rrow[t];
            else if (a.res_mode == AVC_RES_UP2)          // nearest x2 (model.py:61-63)
                w += rrow[t >> 1];
            else if (a.res_mode == AVC_RES_AVGPOOL2) {   // avg_pool1d(2, ceil_mode): the clipped last window divides by 1 (model.py:319)
                const int i0 = 2 * t, i1 = i0 + 1;
                w += (i1 < Tres) ? (rrow[i0] + rrow[i1]) * 0.5f : rrow[i0];
            }
        }
        orow[t] = w;
    }
}

// Backward of rag_instnorm_fwd_kernel: one wavefront per row (b, c), two passes over the row's own T_b frames -- the sums of g and g * xhat
// (per-lane partial sums in frame order, then the fixed butterfly of wave_sum: no atomics), then
// dy = rstd * gamma * (g - mean_t(g) - xhat * mean_t(g * xhat)).  g = G masked by the forward's activation decision: xhat / preact come from
// the SAVED statistics through in_xhat / in_preact, bit for bit the forward's (instnorm_bwd_generic_kernel of rowops.hip).
// ADA = false (the content encoder: gamma = 1, beta = 0): nothing below reads cond / dcond / up, the instance is the kernel the content
// plan always ran.  ADA = true (the decoder's AdaIN rows): gamma / beta from cond in the layout the forward reads; lane 0 stores the row's
// two sums as d(beta), d(gamma) into dcond (same [B][cond_sb] layout; every element written once per pass); up > 1: the PLANAR store behind a
// pixel-shuffling conv (model.py:52-59) -- frame t of row c goes to conv-output row c * up + t % up, frame t / up of the sample's block, which
// is then [C * up][T_b / up]: the conv's input gradient reads a plain stride-1 packed source.
template <bool ADA>
__global__ void __launch_bounds__(AVC_THREADS) rag_instnorm_bwd_kernel(const RagINBwdArgs a) {
    const int tid = threadIdx.x, l = tid & 63;
    const int row = blockIdx.x * 4 + (tid >> 6);
    if (row >= a.B * a.C) return;   // (whole wavefronts leave together: a row is one wavefront)
    const int b = row / a.C, c = row - b * a.C;
    const int T = a.T[b];
    const long base = (long)a.C * a.off[b] + (long)c * T;
    const float* yrow = a.y + base;
    const float* grow = a.g + base;
    const float mean = a.mean[row], rstd = a.rstd[row];
    float gamma = 1.f, beta = 0.f;
    if constexpr (ADA) {
        const float* cr = a.cond + (long)b * a.cond_sb + a.cond_off;
        beta = cr[c];
        gamma = cr[a.C + c];
    }
    float s1 = 0.f, s2 = 0.f;
    for (int t = l; t < T; t += 64) {
        const float h = in_xhat(yrow[t], mean, rstd);
        const float gme = avc_act_grad(grow[t], in_preact(h, gamma, beta) > 0.f, a.slope);
        s1 += gme;
        s2 += gme * h;
    }
    const float invT = 1.0f / (float)T;
    if constexpr (!ADA) {
        const float m1 = wave_sum(s1) * invT, m2 = wave_sum(s2) * invT;
        float* drow = a.dy + base;
        for (int t = l; t < T; t += 64) {
            const float h = in_xhat(yrow[t], mean, rstd);
            const float gme = avc_act_grad(grow[t], in_preact(h, 1.f, 0.f) > 0.f, a.slope);
            drow[t] = rstd * (gme - m1 - h * m2);
        }
    } else {
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        if (l == 0) {
            float* dc = a.dcond + (long)b * a.cond_sb + a.cond_off;
            dc[c] = s1;
            dc[a.C + c] = s2;
        }
        const float m1 = s1 * invT, m2 = s2 * invT, rg = rstd * gamma;
        const int up = a.up > 1 ? a.up : 1, Tc = T / up;   // (T_b is a multiple of up: the level behind an upsampling block)
        float* dblk = a.dy + (long)a.C * a.off[b];
        for (int t = l; t < T; t += 64) {
            const float h = in_xhat(yrow[t], mean, rstd);
            const float gme = avc_act_grad(grow[t], in_preact(h, gamma, beta) > 0.f, a.slope);
            const int tc = t / up;
            dblk[(long)(c * up + (t - tc * up)) * Tc + tc] = rg * (gme - m1 - h * m2);
        }
    }
}

static __device__ __forceinline__ int rag_find(const int* off, int B, int f) {   // sample whose frames [off[b], off[b+1]) hold frame f
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= f) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// raw input last in the concat buffer (model.py:90): dst[b, c0 + m, t] = x[b, m, t]; x is the packed input with explicit
// element strides (xsc, xst) inside a sample's block of M * T_b elements
__global__ void __launch_bounds__(AVC_THREADS)
rag_copy_rows_kernel(const float* x, long xsc, long xst, const int* T, const int* off, int B, int M, int sumT, float* dst, int CC, int c0) {
    const long n = (long)M * sumT;
    for (long e = (long)blockIdx.x * AVC_THREADS + threadIdx.x; e < n; e += (long)gridDim.x * AVC_THREADS) {
        // e = M * off[b] + m * T_b + t  (the order of the destination rows: coalesced stores)
        const int f = (int)(e / M);                 // a frame index inside sample b's block
        const int b = rag_find(off, B, f);
        const long r = e - (long)M * off[b];
        const int Tb = T[b];
        const int m = (int)(r / Tb), t = (int)(r - (long)m * Tb);
        dst[(long)CC * off[b] + (long)(c0 + m) * Tb + t] = x[(long)M * off[b] + (long)m * xsc + (long)t * xst];
    }
}

// AdaptiveAvgPool1d(1) (model.py:273) over each sample's own length -> out[c * B + b] (channel-major for the dense stack)
__global__ void __launch_bounds__(AVC_THREADS) rag_timepool_fwd_kernel(const float* in, const int* T, const int* off, int B, int C, float* out) {
    const int r = blockIdx.x * AVC_THREADS + threadIdx.x;
    if (r >= B * C) return;
    const int b = r / C, c = r - b * C;
    const int Tb = T[b];
    const float* p = in + (long)C * off[b] + (long)c * Tb;
    float s = 0.f;
    for (int t = 0; t < Tb; ++t) s += p[t];
    out[(long)c * B + b] = s / (float)Tb;
}

// backward of the pooling + activation mask of the last block, the ragged twin of timepool_bwd_kernel (rowops.hip): every frame of
// sample b's row c gets G = dP[c][b] / T_b; dy = G masked by the block's saved activation.  Packed [C][T_b] blocks.
__global__ void __launch_bounds__(AVC_THREADS)
rag_timepool_bwd_kernel(const float* dP, const float* amask, const int* T, const int* off, int B, int C, int sumT, float* G, float* dy, float slope) {
    const long n = (long)C * sumT;
    for (long e = (long)blockIdx.x * AVC_THREADS + threadIdx.x; e < n; e += (long)gridDim.x * AVC_THREADS) {
        const int f = (int)(e / C);   // a frame index inside sample b's block (the block starts at element C * off[b])
        const int b = rag_find(off, B, f);
        const int Tb = T[b];
        const int c = (int)((e - (long)C * off[b]) / Tb);
        const float gv = dP[(long)c * B + b] / (float)Tb;
        if (G) G[e] = gv;
        if (dy) dy[e] = avc_act_grad(gv, amask[e] > 0.f, slope);
    }
}

// dst[c][r] = src[r * sr + c * sc]: the caller's strided d(emb) [B, c_cond] -> the dense stack's channel-major operand
__global__ void __launch_bounds__(AVC_THREADS) transpose_strided_kernel(float* dst, const float* src, long sr, long sc, int R, int C) {
    const int e = blockIdx.x * AVC_THREADS + threadIdx.x;
    if (e >= R * C) return;
    const int c = e / R, r = e - c * R;
    dst[e] = src[(long)r * sr + (long)c * sc];
}

int avc_launch_rag_timepool_bwd(const float* dP, const float* amask, const int* T, const int* off, int B, int C, int sumT, float* G, float* dy,
                                float slope, hipStream_t s) {
    const long n = (long)C * sumT;
    long blocks = (n + AVC_THREADS - 1) / AVC_THREADS;
    if (blocks > 2048) blocks = 2048;
    ProfScope ps(AVC_K_MISC, 0.0, 0.0, s);
    hipLaunchKernelGGL(rag_timepool_bwd_kernel, dim3((int)blocks), dim3(AVC_THREADS), 0, s, dP, amask, T, off, B, C, sumT, G, dy, slope);
    return (int)hipGetLastError();
}
int avc_launch_transpose_strided(float* dst, const float* src, long sr, long sc, int R, int C, hipStream_t s) {
    ProfScope ps(AVC_K_MISC, 0.0, 0.0, s);
    hipLaunchKernelGGL(transpose_strided_kernel, dim3(avc_cdiv(R * C, AVC_THREADS)), dim3(AVC_THREADS), 0, s, dst, src, sr, sc, R, C);
    return (int)hipGetLastError();
}

int avc_launch_rag_in_fwd(const RagINArgs& a, hipStream_t s) {
    ProfScope ps(AVC_K_IN_FWD, 0.0, 0.0, s);
    hipLaunchKernelGGL(rag_instnorm_fwd_kernel, dim3(avc_cdiv(a.B * a.C, 4)), dim3(AVC_THREADS), 0, s, a);
    return (int)hipGetLastError();
}
int avc_launch_rag_in_bwd(const RagINBwdArgs& a, hipStream_t s) {
    ProfScope ps(AVC_K_IN_BWD, 0.0, 0.0, s);
    if (a.cond) hipLaunchKernelGGL((rag_instnorm_bwd_kernel<true>), dim3(avc_cdiv(a.B * a.C, 4)), dim3(AVC_THREADS), 0, s, a);
    else hipLaunchKernelGGL((rag_instnorm_bwd_kernel<false>), dim3(avc_cdiv(a.B * a.C, 4)), dim3(AVC_THREADS), 0, s, a);
    return (int)hipGetLastError();
}
int avc_launch_rag_copy_rows(const float* x, long xsc, long xst, const int* T, const int* off, int B, int M, int sumT, float* dst, int CC, int c0,
                             hipStream_t s) {
    long n = (long)M * sumT;
    long blocks = (n + AVC_THREADS - 1) / AVC_THREADS;
    if (blocks > 2048) blocks = 2048;
    ProfScope ps(AVC_K_MISC, 0.0, 0.0, s);
    hipLaunchKernelGGL(rag_copy_rows_kernel, dim3((int)blocks), dim3(AVC_THREADS), 0, s, x, xsc, xst, T, off, B, M, sumT, dst, CC, c0);
    return (int)hipGetLastError();
}
int avc_launch_rag_timepool_fwd(const float* in, const int* T, const int* off, int B, int C, float* out, hipStream_t s) {
    ProfScope ps(AVC_K_MISC, 0.0, 0.0, s);
    hipLaunchKernelGGL(rag_timepool_fwd_kernel, dim3(avc_cdiv(B * C, AVC_THREADS)), dim3(AVC_THREADS), 0, s, in, T, off, B, C, out);
    return (int)hipGetLastError();
}
