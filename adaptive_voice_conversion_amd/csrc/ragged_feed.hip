// Device-side feed of the ragged training step: whole utterances (or crops of them) of DIFFERENT lengths out of the HBM-resident corpus
// [n_rows][M] into the frame-major packed block the ragged grad plans and avc_loss_ragged read.  The ragged counterpart of
// gather_segments_kernel of rowops.hip; C ABI at the end of the file (include/avc_hip.h: avc_gather_utterances).
//
// Layouts:
//   corpus   [n_rows][M] fp32, mel bins contiguous
//   out      utterance j = rows [T_j][M] at row xoff[j] = sum T[0..j): out[(xoff[j] + t) M + m] = corpus[(starts[j] + t) M + m]
// Both sides of utterance j are ONE contiguous run of T_j M floats, so this is a segmented copy with no transpose and no LDS: lanes walk
// the run with unit stride.  Where the run starts on a 16-byte boundary on both sides (starts[j] M and xoff[j] M multiples of 4, both base
// pointers 16-byte aligned) a lane moves 16 bytes per access (global_load_dwordx4 / global_store_dwordx4: 1 KiB per wavefront
// instruction) and the n % 4 floats left over go one by one; otherwise every lane moves 4 bytes.  The test is per utterance and uniform
// over a workgroup.  starts / T / xoff are DEVICE tables: the launch needs nothing from the host but its scalar arguments.
#include <hip/hip_runtime.h>

#include "avc_common.h"
#include "avc_internal.h"

#define GU_VPT 4                              // 16-byte accesses of one lane in the vector path
#define GU_TILE (AVC_THREADS * GU_VPT * 4)    // floats of one workgroup's piece of a run (16 KiB)

// grid (pieces of GU_TILE floats of the LONGEST run, N): a workgroup beyond its utterance's T_j M floats exits.  An utterance whose rows
// are not all inside the corpus is left out as a whole (nothing of it is read, nothing of its block is written).
__global__ void __launch_bounds__(AVC_THREADS)
gather_utterances_kernel(const float* corpus, long n_rows, int M, const long* starts, const int* T, const int* xoff, int base_vec, float* out) {
    const int j = blockIdx.y, tid = threadIdx.x;
    const long st = starts[j];
    const int Tj = T[j];
    if (Tj < 1 || st < 0 || st > n_rows - Tj) return;   // (the whole workgroup leaves together)
    const long n = (long)Tj * M;
    const long p0 = (long)blockIdx.x * GU_TILE;
    if (p0 >= n) return;
    const long so = st * M, dof = (long)xoff[j] * M;
    const float* src = corpus + so;
    float* dst = out + dof;
    if (base_vec && ((so | dof) & 3) == 0) {
        const long nv = n >> 2;
        const float4* s4 = (const float4*)src;
        float4* d4 = (float4*)dst;
        const long v0 = p0 >> 2;
        float4 r[GU_VPT];
#pragma unroll
        for (int k = 0; k < GU_VPT; ++k) {   // all loads first: GU_VPT independent requests in flight per lane
            const long v = v0 + k * AVC_THREADS + tid;
            if (v < nv) r[k] = s4[v];
        }
#pragma unroll
        for (int k = 0; k < GU_VPT; ++k) {
            const long v = v0 + k * AVC_THREADS + tid;
            if (v < nv) d4[v] = r[k];
        }
        if (blockIdx.x == 0 && tid < (int)(n & 3)) dst[(nv << 2) + tid] = src[(nv << 2) + tid];   // the n % 4 floats behind the last vector
        return;
    }
    const long p1 = (p0 + GU_TILE < n) ? p0 + GU_TILE : n;
    for (long e = p0 + tid; e < p1; e += AVC_THREADS) dst[e] = src[e];
}

extern "C" {
int avc_gather_utterances(const float* corpus, long n_rows, int M, const long* starts_dev, const int* T_dev, const int* xoff_dev, int N, int T_max,
                          float* out, void* stream) {
    if (!corpus || !starts_dev || !T_dev || !xoff_dev || !out) return -1;
    if (n_rows < 1 || M < 1 || N < 1 || N > 65535 || T_max < 1) return -1;
    const long pieces = ((long)T_max * M + GU_TILE - 1) / GU_TILE;
    if (pieces > 0x7fffffffL) return -1;
    const int base_vec = ((((unsigned long)corpus) | ((unsigned long)out)) & 15) == 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(AVC_K_MISC, 0.0, 0.0, s);
    hipLaunchKernelGGL(gather_utterances_kernel, dim3((unsigned)pieces, (unsigned)N), dim3(AVC_THREADS), 0, s, corpus, n_rows, M, starts_dev, T_dev,
                       xoff_dev, base_vec, out);
    return (int)hipGetLastError();
}
}
