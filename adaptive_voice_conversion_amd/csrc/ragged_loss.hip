// Loss-side kernels of a training step over utterances of DIFFERENT lengths (solver.py:84-86 and model.py:383-384 on the packed rows
// of the ragged plans): the reparameterisation z = mu + exp(log_sigma / 2) * eps, the L1 + KL loss with d(loss)/d(dec), and d(loss)/d(mu |
// log_sigma) from the KL term and from d(z).  The ragged counterparts of reparam_fwd_kernel / loss_partial_kernel / loss_final_kernel /
// latent_bwd_kernel of rowops.hip; C ABI at the end of the file (include/avc_hip.h: avc_reparam_ragged, avc_loss_ragged,
// avc_latent_bwd_ragged).
//
// Layouts (those of the ragged plans):
//   x        utterance j = rows [T_j][M] (mel bins contiguous) at row xoff[j] = sum T[0..j)
//   dec      block j = [M][T''_j] (frames contiguous) at float offset out_off[j]; T''_j >= T_j is the decoder's own output length
//   muls     block s = [2 c][Tz_s] at 2 c offz[s], the c mu rows first, then the c log_sigma rows
//   z / eps  block s = [c][Tz_s] at c offz[s]
// Lengths and offsets are DEVICE tables the caller built once per tuple of lengths: no launch below needs anything from the host but its
// scalar arguments.  fp32, no atomics, a fixed summation order: two calls give identical bits.
#include <hip/hip_runtime.h>

#include "avc_common.h"
#include "avc_internal.h"

#define RL_TF 64      // frames of one loss tile
#define RL_MC 64      // mel bins staged per pass over the tile (the kernel loops over ceil(M / RL_MC) chunks: LDS does not grow with M)
#define RL_PITCH 65   // odd row pitch of the staged [RL_TF][RL_MC] tile (dwords)

static __device__ __forceinline__ float rl_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// block_sum of rowops.hip: the butterfly inside each wavefront, then the four wavefronts in a fixed order
static __device__ __forceinline__ float rl_block_sum(float v, float* red) {
    v = rl_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// z = mu + exp(log_sigma / 2) * eps (model.py:383-384), reparam_fwd_kernel's expression; eps == NULL: z = mu.
// grid (tiles of AVC_THREADS elements of the LONGEST block, S): a workgroup beyond its sample's c * Tz_s elements exits.
__global__ void __launch_bounds__(AVC_THREADS)
rag_reparam_kernel(const float* muls, const float* eps, const int* Tz, const int* offz, int c, float* z) {
    const int s = blockIdx.y;
    const long per = (long)c * Tz[s];
    const long i = (long)blockIdx.x * AVC_THREADS + threadIdx.x;
    if (i >= per) return;
    const long zb = (long)c * offz[s];
    const float* mb = muls + 2 * zb;
    const float mu = mb[i], ls = mb[per + i];
    z[zb + i] = eps ? mu + expf(ls * 0.5f) * eps[zb + i] : mu;
}

// d(muls) from the KL term (solver.py:86) and from z (model.py:384), latent_bwd_kernel's expressions in its order:
//   dmu = lkl/N * mu + dz ;  dls = lkl/N * 0.5 * (exp(ls) - 1) + dz * eps * 0.5 * exp(ls / 2)     (eps == NULL: no second term of dls)
// Every product and sum is rounded on its own (no contraction into fused multiply-adds): the eps == NULL result is, bit for bit, what the
// two formulas give when evaluated one fp32 operation at a time.  Grid as rag_reparam_kernel.
__global__ void __launch_bounds__(AVC_THREADS)
rag_latent_bwd_kernel(const float* muls, const float* eps, const float* dz, const int* Tz, const int* offz, int c, float lambda_kl_over_n,
                      float* dmuls) {
#pragma clang fp contract(off)
    const int s = blockIdx.y;
    const long per = (long)c * Tz[s];
    const long i = (long)blockIdx.x * AVC_THREADS + threadIdx.x;
    if (i >= per) return;
    const long zb = (long)c * offz[s];
    const float* mb = muls + 2 * zb;
    float* db = dmuls + 2 * zb;
    const float mu = mb[i], ls = mb[per + i];
    const float dzv = dz[zb + i];
    const float dmu = lambda_kl_over_n * mu + dzv;
    float dls = lambda_kl_over_n * 0.5f * (expf(ls) - 1.0f);
    if (eps) dls = dls + dzv * eps[zb + i] * 0.5f * expf(ls * 0.5f);
    db[i] = dmu;
    db[per + i] = dls;
}

// L1 + KL partial sums (solver.py:84-86) and d(dec) = scale * sign(dec - x) on the CROPPED rows: frames t < T_j of output block j count,
// the crop tail T_j <= t < T''_j gets d(dec) = 0 and adds nothing.  One workgroup = (utterance j, tile of RL_TF frames); grid (ntile_max, N),
// a workgroup beyond its utterance's ceil(T''_j / RL_TF) tiles stores two zeros and exits.
// x is frame-major, dec channel-major: per chunk of RL_MC mel bins the [RL_TF][RL_MC] tile of x is read with lanes along the mel axis
// (coalesced), staged in LDS at row pitch RL_PITCH, and read back transposed with lanes along the frames, the direction dec / d_dec are
// walked in (coalesced).  Banks (ds_write_b32 / ds_read_b32: 32 banks, conflicts inside a 32-lane half): the store puts a half on 32
// consecutive dwords of one row; the transposed read puts it on dwords lane * 65 + m, bank (lane + m) % 32 -- both conflict-free.
// Every element of d(dec) block j is written exactly once.  The same workgroups share the KL sum of latent block j among the tiles of
// utterance j (element i goes to tile (i / AVC_THREADS) % ntile_j).  partial[2 (j ntile_max + tile)] = {L1 sum, KL sum}.
__global__ void __launch_bounds__(AVC_THREADS)
rag_loss_kernel(const float* dec, const int* out_len, const long* out_off, const float* x, const int* T, const int* xoff, int M, int ntile_max,
                const float* muls, const int* Tz, const int* offz, int c, float scale, float* ddec, float* partial) {
    __shared__ float tile[RL_TF * RL_PITCH];
    __shared__ float red[4];
    const int j = blockIdx.y, tl = blockIdx.x, tid = threadIdx.x;
    const int l = tid & 63, w = tid >> 6;
    const int Tj = T[j], Tpp = out_len[j];
    const int ntile = (Tpp + RL_TF - 1) / RL_TF;
    float* pout = partial + 2 * ((long)j * ntile_max + tl);
    if (tl >= ntile) {   // (the whole workgroup leaves together)
        if (tid == 0) {
            pout[0] = 0.f;
            pout[1] = 0.f;
        }
        return;
    }
    const int t0 = tl * RL_TF;
    const float* xj = x + (long)xoff[j] * M;
    const float* dj = dec + out_off[j];
    float* gj = ddec + out_off[j];
    float s = 0.f;
    for (int m0 = 0; m0 < M; m0 += RL_MC) {
        __syncthreads();   // (the previous chunk's transposed reads are done)
        for (int f = w; f < RL_TF; f += AVC_THREADS / 64) {
            const int t = t0 + f, m = m0 + l;
            tile[f * RL_PITCH + l] = (t < Tj && m < M) ? xj[(long)t * M + m] : 0.f;
        }
        __syncthreads();
        const int t = t0 + l;
        if (t < Tpp) {
            for (int mm = w; mm < RL_MC && m0 + mm < M; mm += AVC_THREADS / 64) {
                const long e = (long)(m0 + mm) * Tpp + t;
                float g = 0.f;
                if (t < Tj) {
                    const float d = dj[e] - tile[l * RL_PITCH + mm];
                    s += fabsf(d);
                    g = (d > 0.f) ? scale : ((d < 0.f) ? -scale : 0.f);
                }
                gj[e] = g;
            }
        }
    }
    float k = 0.f;
    const long per = (long)c * Tz[j];
    const float* mb = muls + 2L * c * offz[j];
    for (long i = (long)tl * AVC_THREADS + tid; i < per; i += (long)ntile * AVC_THREADS) {
        const float mu = mb[i], ls = mb[per + i];
        k += expf(ls) + mu * mu - 1.0f - ls;
    }
    const float bs = rl_block_sum(s, red);
    const float bk = rl_block_sum(k, red);
    if (tid == 0) {
        pout[0] = bs;
        pout[1] = bk;
    }
}

// the two means out of the partial sums, loss_final_kernel's order: thread i sums partials i, i + AVC_THREADS, ... in index order, then the
// fixed block sum
__global__ void __launch_bounds__(AVC_THREADS)
rag_loss_final_kernel(const float* partial, int nparts, float inv_n_rec, float half_inv_n_kl, float* losses) {
    __shared__ float red[4];
    float s = 0.f, k = 0.f;
    for (int i = threadIdx.x; i < nparts; i += AVC_THREADS) {
        s += partial[2 * i];
        k += partial[2 * i + 1];
    }
    const float ts = rl_block_sum(s, red);
    const float tk = rl_block_sum(k, red);
    if (threadIdx.x == 0) {
        losses[0] = ts * inv_n_rec;        // loss_rec = mean |dec - x| over the kept elements
        losses[1] = tk * half_inv_n_kl;    // loss_kl = 0.5 * mean(exp(ls) + mu^2 - 1 - ls)
    }
}

static bool rl_latent_grid(int S, int Tz_max, int c, dim3* grid) {
    if (S < 1 || S > 65535 || Tz_max < 1 || c < 1) return false;
    const long tiles = ((long)c * Tz_max + AVC_THREADS - 1) / AVC_THREADS;
    if (tiles > 0x7fffffffL) return false;
    *grid = dim3((unsigned)tiles, (unsigned)S);
    return true;
}

static long rl_ntile_max(int T_max) { return ((long)T_max + RL_TF - 1) / RL_TF; }

extern "C" {
int avc_reparam_ragged(const float* muls, const float* eps, int S, const int* Tz_dev, const int* offz_dev, int Tz_max, int c, float* z,
                       void* stream) {
    dim3 grid;
    if (!muls || !Tz_dev || !offz_dev || !z || !rl_latent_grid(S, Tz_max, c, &grid)) return -1;
    ProfScope ps(AVC_K_MISC, 0.0, 0.0, (hipStream_t)stream);
    hipLaunchKernelGGL(rag_reparam_kernel, grid, dim3(AVC_THREADS), 0, (hipStream_t)stream, muls, eps, Tz_dev, offz_dev, c, z);
    return (int)hipGetLastError();
}

long avc_loss_ragged_ws_floats(int N, int T_max) {
    if (N < 1 || N > 65535 || T_max < 1) return -1;
    const long n = 2L * N * rl_ntile_max(T_max);
    return n > 0x7fffffffL ? -1 : n;
}

int avc_loss_ragged(const float* dec, const int* out_len_dev, const long* out_off_dev, const float* x, const int* T_dev, const int* xoff_dev, int N,
                    int M, int T_max, const float* muls, const int* Tz_dev, const int* offz_dev, int c, long n_rec, long n_kl, float lambda_rec,
                    float* d_dec, float* losses, float* ws, void* stream) {
    if (!dec || !out_len_dev || !out_off_dev || !x || !T_dev || !xoff_dev || !muls || !Tz_dev || !offz_dev || !d_dec || !losses || !ws) return -1;
    if (M < 1 || c < 1 || n_rec < 1 || n_kl < 1 || avc_loss_ragged_ws_floats(N, T_max) < 0) return -1;
    const int ntile_max = (int)rl_ntile_max(T_max);
    const float scale = (float)((double)lambda_rec / (double)n_rec);   // one rounding
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(AVC_K_MISC, 0.0, 0.0, s);
    hipLaunchKernelGGL(rag_loss_kernel, dim3(ntile_max, N), dim3(AVC_THREADS), 0, s, dec, out_len_dev, out_off_dev, x, T_dev, xoff_dev, M, ntile_max,
                       muls, Tz_dev, offz_dev, c, scale, d_dec, ws);
    hipLaunchKernelGGL(rag_loss_final_kernel, dim3(1), dim3(AVC_THREADS), 0, s, ws, N * ntile_max, (float)(1.0 / (double)n_rec),
                       (float)(0.5 / (double)n_kl), losses);
    return (int)hipGetLastError();
}

int avc_latent_bwd_ragged(const float* muls, const float* eps, const float* d_z, int S, const int* Tz_dev, const int* offz_dev, int Tz_max, int c,
                          float lambda_kl_over_n, float* d_muls, void* stream) {
    dim3 grid;
    if (!muls || !d_z || !Tz_dev || !offz_dev || !d_muls || !rl_latent_grid(S, Tz_max, c, &grid)) return -1;
    ProfScope ps(AVC_K_MISC, 0.0, 0.0, (hipStream_t)stream);
    hipLaunchKernelGGL(rag_latent_bwd_kernel, grid, dim3(AVC_THREADS), 0, (hipStream_t)stream, muls, eps, d_z, Tz_dev, offz_dev, c, lambda_kl_over_n,
                       d_muls);
    return (int)hipGetLastError();
}
}
