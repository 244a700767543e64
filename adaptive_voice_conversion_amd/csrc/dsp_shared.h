// Device code shared by the single-utterance DSP kernels (dsp.hip) and their packed, many-utterance twins (dsp_ragged.hip): the two
// files are separate translation units, and a ragged kernel is bit-equal to its single twin BY CONSTRUCTION when both call the same
// inline on the same utterance (same lane partition, same reduction tree, same carry sequence, same arithmetic expression).
#pragma once
#include <hip/hip_runtime.h>

#include "avc_common.h"

static inline int dsp_blocks(long n) {
    long b = (n + AVC_THREADS - 1) / AVC_THREADS;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// numpy.pad(mode='reflect') index for a pad shorter than the signal
static __device__ __forceinline__ long dsp_reflect(long v, long L) {
    if (v < 0) v = -v;
    if (v >= L) v = 2 * (L - 1) - v;
    return v;
}

// largest b in [0, B) with start(b) <= key; start(b) = toff[b] (frames), or hop (toff[b] - b) (samples of the Griffin-Lim packing)
static __device__ __forceinline__ int dsp_find(const int* toff, int B, long key, int hop, bool samples) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const long start = samples ? (long)hop * (toff[mid] - mid) : (long)toff[mid];
        if (start <= key) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// utils.py:60 at sample i of the signal that STARTS at y: out[0] = y[0], out[i] = y[i] - a y[i-1]
static __device__ __forceinline__ float dsp_preemph_at(const float* y, long i, float a) { return i == 0 ? y[0] : y[i] - a * y[i - 1]; }

// One workgroup of AVC_THREADS lanes: mean square of frame `fr` of the signal y[0 .. L) (librosa.feature.rms, center=True) -> *out.
// red: AVC_THREADS floats of LDS.
static __device__ __forceinline__ void dsp_frame_power_body(const float* y, long L, int frame_length, int hop, long fr, float* red, float* out) {
    float s = 0.f;
    for (int k = threadIdx.x; k < frame_length; k += AVC_THREADS) {
        const float v = y[dsp_reflect(fr * hop + k - frame_length / 2, L)];
        s += v * v;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = AVC_THREADS / 2; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0] / (float)frame_length;
}

// One workgroup of 1024 lanes: out[i] = x[i] + a out[i-1] over x[0 .. L).  Each lane a contiguous run of (L + 1023) / 1024 samples:
// local recurrence, then the carries in sequence (1024 steps), then out += a^(j+1) * carry_in.  last / cin / apow: 1024 floats of LDS each.
static __device__ __forceinline__ void dsp_deemph_body(const float* x, long L, float a, float* out, float* last, float* cin, float* apow) {
    const int tid = threadIdx.x;
    const long run = (L + 1023) / 1024;
    const long i0 = (long)tid * run, i1 = (i0 + run < L) ? i0 + run : L;
    float v = 0.f, p = 1.f;
    for (long i = i0; i < i1; ++i) {
        v = x[i] + a * v;
        out[i] = v;
        p *= a;
    }
    last[tid] = v;
    apow[tid] = p;
    __syncthreads();
    if (tid == 0) {
        float c = 0.f;
        for (int j = 0; j < 1024; ++j) {
            cin[j] = c;
            c = last[j] + apow[j] * c;
        }
    }
    __syncthreads();
    const float c = cin[tid];
    if (c != 0.f) {
        float q = a;
        for (long i = i0; i < i1; ++i) {
            out[i] += q * c;
            q *= a;
        }
    }
}
