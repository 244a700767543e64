// Conv1d weight gradient over packed rows of UNEQUAL length (the ragged speaker encoder's parameter gradients, avc_backward_ragged_params,
// and the op-level avc_conv1d_wgrad_ragged):
//     dW[co][ci][j] = sum_b sum_t dy_b[co][t] * xpad_b[ci][t * stride + j],      db[co] = sum_b sum_t dy_b[co][t]
// xpad_b = sample b's own reflect padding (k / 2 left; k / 2 right for odd k, k / 2 - 1 for even k: pad_layer, model.py:21-32).
//
// GEMM view: M = co, N = (ci, tap), K = (b, t).  A kernel of its own, not an instance of conv_wgrad.hip: K is a few hundred to a few
// thousand frames here, the launches are latency-bound, and the stream-K walk, the producer waves and the LDS-DMA pipeline of the uniform
// kernel buy nothing at that size.  What it keeps from there: fp32 MFMA products (v_mfma_f32_32x32x2_f32), a fixed summation order, split-K
// partials in slots that a second launch sums in slot order, no atomics.
//
// Tile: 64 co x 64 ci x all taps per workgroup of four waves (2 x 2 blocks of 32 x 32, KS accumulators of 16 registers per wave; the
// eight-tap bank member holds 128).  K-chunk: 32 output frames of ONE sample, from a device table of (sample, first frame) built where the
// level tables are built -- a chunk never straddles a block boundary, and the ragged tail of a sample's last chunk is staged as zeros
// in dy, so whatever x holds there is multiplied by zero.  Per chunk the workgroup stages
//     dy  [64 co][32 t]                     rows of 33 floats
//     x   [64 ci][31 stride + KS frames]    rows of 71 floats, reflected at THAT sample's edges while it is staged (a sample so short
//                                           that both mirror windows fall into one chunk, the last frame of an odd row under stride 2)
// with plain coalesced loads (frames contiguous), then every wave reads its A fragment (dy, lane = row, the two lane halves = two
// consecutive frames) once per k-step and one B fragment per tap.  Odd row strides: the 32 lanes of a ds_read_b32 group read 32
// consecutive rows at one column -> 32 different banks (33 = 1, 71 = 7 mod 32).
//
// Fixed order: a workgroup walks its chunks in table order, frames in ascending order inside the MFMA chain; slots are summed in
// ascending slot order by rwg_reduce_kernel.  Two passes give identical bits.
#include <hip/hip_runtime.h>

#include <vector>

#include "avc_common.h"
#include "avc_internal.h"

#define RWG_THREADS 256
#define RWG_DYROW 33
#define RWG_XROW 71   // >= 31 * 2 + 8, odd

// SJ: a STRIDED one-sample job (RagWgJob::strided; KS = 1, stride = 1): only the staging differs -- the chunks, the MFMA chain, the slots and
// the stores are the packed job's, so at packed strides the two give the same bits.
template <int KS, bool SJ = false>
static __device__ __forceinline__ void rwg_body(const RagWgJob& J, int local, float* sdy, float* sx) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, h = lane >> 5;
    const int co_tiles = avc_cdiv(J.Cout, 64);
    const int tiles = co_tiles * J.ci_tiles;
    const int z = local / tiles, tile = local - z * tiles;
    const int co0 = (tile / J.ci_tiles) * 64, ci0 = (tile % J.ci_tiles) * 64;
    const int wm = wave & 1, wn = wave >> 1;
    const bool active = (co0 + wm * 32 < J.Cout) && (ci0 + wn * 32 < J.Cin);   // wave-uniform: a block of padding rows multiplies nothing
    const bool bias_wg = (ci0 == 0);
    const int c_lo = (int)(((long)z * J.nchunks) / J.nsplit), c_hi = (int)(((long)(z + 1) * J.nchunks) / J.nsplit);
    const int stride = J.stride, padL = KS / 2;
    const int XSEG = 31 * stride + KS;

    f32x16 acc[KS];
#pragma unroll
    for (int j = 0; j < KS; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    float bsum = 0.f;

    for (int c = c_lo; c < c_hi; ++c) {
        if constexpr (SJ) {
            // No tables, no reflection (KS = 1): chunk c = frames [32 c, 32 c + 32) of the one sample.  The lane order of each staging loop
            // follows the operand's unit-stride axis, so a wave's loads stay coalesced: channels fastest where the channel stride is 1
            // (frame-major d(cond), a row-major emb, an expanded single voice), frames fastest otherwise.  The LDS rows keep their odd strides:
            // 32 consecutive channels at one frame fall into 32 different banks (33 = 1, 71 = 7 mod 32), as 32 consecutive frames of a row do.
            const int t0 = 32 * c, N = J.nframes;
            const bool ych = (J.syc == 1 && J.syt != 1), xch = (J.sxc == 1 && J.sxt != 1);   // block-uniform
            for (int i = tid; i < 64 * 32; i += RWG_THREADS) {
                const int r = ych ? (i & 63) : (i >> 5), t = ych ? (i >> 6) : (i & 31);
                const int co = co0 + r, tt = t0 + t;
                sdy[r * RWG_DYROW + t] = (co < J.Cout && tt < N) ? J.dy[(long)co * J.syc + (long)tt * J.syt] : 0.f;
            }
            for (int i = tid; i < 64 * 32; i += RWG_THREADS) {
                const int r = xch ? (i & 63) : (i >> 5), q = xch ? (i >> 6) : (i & 31);
                const int ci = ci0 + r, f = t0 + q;
                sx[r * RWG_XROW + q] = (ci < J.Cin && f < N) ? J.x[(long)ci * J.sxc + (long)f * J.sxt] : 0.f;
            }
        } else {
            const int b = J.chunk[2 * c], t0 = J.chunk[2 * c + 1];
            const int Tin = J.Tin[b], Tout = J.Tout[b];
            const float* xb = J.x + (long)J.xC * J.offin[b] + (long)J.xc0 * Tin;
            const float* yb = J.dy + (long)J.dyC * J.offout[b] + (long)J.dyc0 * Tout;
            for (int i = tid; i < 64 * 32; i += RWG_THREADS) {
                const int r = i >> 5, t = i & 31;
                const int co = co0 + r, tt = t0 + t;
                sdy[r * RWG_DYROW + t] = (co < J.Cout && tt < Tout) ? yb[(long)co * Tout + tt] : 0.f;
            }
            for (int i = tid; i < 64 * XSEG; i += RWG_THREADS) {
                const int r = i / XSEG, q = i - r * XSEG;
                const int ci = ci0 + r;
                int f = t0 * stride + q - padL;
                f = f < 0 ? -f : f;
                f = f >= Tin ? 2 * (Tin - 1) - f : f;
                // (a frame still outside after one reflection belongs to output frames past the sample's end: dy is zero there)
                sx[r * RWG_XROW + q] = (ci < J.Cin && f >= 0 && f < Tin) ? xb[(long)ci * Tin + f] : 0.f;
            }
        }
        __syncthreads();
        if (active) {
            const float* ar = sdy + (wm * 32 + li) * RWG_DYROW + h;
            const float* br = sx + (wn * 32 + li) * RWG_XROW + h * stride;
#pragma unroll 4
            for (int kk = 0; kk < 16; ++kk) {
                const float a = ar[2 * kk];
#pragma unroll
                for (int j = 0; j < KS; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, br[2 * kk * stride + j], acc[j], 0, 0, 0);
            }
        }
        if (bias_wg && tid < 64) {
            const float* row = sdy + tid * RWG_DYROW;
#pragma unroll 8
            for (int t = 0; t < 32; ++t) bsum += row[t];
        }
        __syncthreads();
    }

    const long n_w = (long)J.Cout * J.Cin * KS;
    float* out = J.out + (J.nsplit > 1 ? (long)z * J.slot_floats : 0);
    if (active) {
        const int ci = ci0 + wn * 32 + li;
        if (ci < J.Cin) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (co < J.Cout) {
#pragma unroll
                    for (int j = 0; j < KS; ++j) out[((long)co * J.Cin + ci) * KS + j] = acc[j][r];
                }
            }
        }
    }
    if (bias_wg && tid < 64 && co0 + tid < J.Cout) {
        if (J.nsplit > 1) out[n_w + co0 + tid] = bsum;
        else if (J.db) J.db[co0 + tid] = bsum;
    }
}

__global__ void __launch_bounds__(RWG_THREADS) conv_wgrad_ragged_kernel(const RagWgArgs A) {
    __shared__ float sdy[64 * RWG_DYROW];
    __shared__ float sx[64 * RWG_XROW];
    int ji = 0;
    for (int i = 1; i < A.njobs; ++i) ji = ((int)blockIdx.x >= A.j[i].wg_begin) ? i : ji;
    const RagWgJob& J = A.j[ji];
    const int local = (int)blockIdx.x - J.wg_begin;
    if (J.strided) {   // (block-uniform, like the tap count below)
        rwg_body<1, true>(J, local, sdy, sx);
        return;
    }
    switch (J.KS) {   // (block-uniform: the taps are a compile-time count inside, the accumulators stay in registers)
        case 1: rwg_body<1>(J, local, sdy, sx); break;
        case 2: rwg_body<2>(J, local, sdy, sx); break;
        case 3: rwg_body<3>(J, local, sdy, sx); break;
        case 4: rwg_body<4>(J, local, sdy, sx); break;
        case 5: rwg_body<5>(J, local, sdy, sx); break;
        case 6: rwg_body<6>(J, local, sdy, sx); break;
        case 7: rwg_body<7>(J, local, sdy, sx); break;
        default: rwg_body<8>(J, local, sdy, sx); break;
    }
}

__global__ void __launch_bounds__(RWG_THREADS) rwg_reduce_kernel(const RagWgRedArgs R) {
    int k = 0;
    for (int i = 1; i < R.n; ++i) k = ((int)blockIdx.x >= R.it[i].blk_begin) ? i : k;
    const RagWgRed& a = R.it[k];
    const long i = (long)((int)blockIdx.x - a.blk_begin) * RWG_THREADS + threadIdx.x;
    if (i >= a.n_w + a.n_b) return;
    const float* p = a.slab + i;
    float v = 0.f;
    for (int z = 0; z < a.nsplit; ++z) v += p[(long)z * a.slot_floats];
    if (i < a.n_w) a.dw[i] = v;
    else if (a.db) a.db[i - a.n_w] = v;
}

// Split of a layer's K axis: a workgroup walks at least four chunks, a layer is split at most 16 ways (its reduce reads 16 slots per
// element) and never into more than about 256 workgroups.
int avc_rwg_nsplit(int Cin, int Cout, int nchunks) {
    const int tiles = avc_cdiv(Cout, 64) * avc_cdiv(Cin, 64);
    int n = nchunks / 4;
    n = n > 16 ? 16 : n;
    const int cap = 256 / tiles;
    n = n > cap ? cap : n;
    return n < 1 ? 1 : n;
}
long avc_rwg_slot_floats(int Cin, int Cout, int KS) { return ((long)Cout * Cin * KS + Cout + 63) / 64 * 64; }

int avc_launch_rwg(RagWgJob* jobs, int n, hipStream_t s) {
    for (int i0 = 0; i0 < n; i0 += AVC_RWG_MAXJ) {
        RagWgArgs A;
        memset(&A, 0, sizeof(A));
        int wgs = 0;
        double flops = 0;
        for (int i = i0; i < n && i < i0 + AVC_RWG_MAXJ; ++i) {
            RagWgJob& j = jobs[i];
            if (j.KS < 1 || j.KS > 8 || j.stride < 1 || j.stride > 2 || j.nsplit < 1 || j.nchunks < 1 || j.Cin < 1 || j.Cout < 1) return -1;
            if (j.nsplit > j.nchunks || (j.nsplit > 1 && j.slot_floats < (long)j.Cout * j.Cin * j.KS + j.Cout)) return -1;
            if (j.strided && (j.KS != 1 || j.stride != 1 || j.nframes < 1 || j.nchunks != avc_cdiv(j.nframes, 32) || j.sxc < 0 || j.sxt < 0 ||
                              j.syc < 0 || j.syt < 0))
                return -1;
            j.ci_tiles = avc_cdiv(j.Cin, 64);
            j.wg_begin = wgs;
            wgs += avc_cdiv(j.Cout, 64) * j.ci_tiles * j.nsplit;
            flops += 2.0 * j.Cout * j.Cin * j.KS * 32.0 * j.nchunks;
            A.j[A.njobs++] = j;
        }
        ProfScope ps(AVC_K_CONV_WGRAD, flops, 0.0, s);
        hipLaunchKernelGGL(conv_wgrad_ragged_kernel, dim3(wgs), dim3(RWG_THREADS), 0, s, A);
        if (int rc = (int)hipGetLastError()) return rc;
    }
    return 0;
}

int avc_launch_rwg_reduce(const RagWgRed* it, int n, hipStream_t s) {
    for (int i0 = 0; i0 < n; i0 += AVC_RWG_MAXR) {
        RagWgRedArgs R;
        memset(&R, 0, sizeof(R));
        int blocks = 0;
        double bytes = 0;
        for (int i = i0; i < n && i < i0 + AVC_RWG_MAXR; ++i) {
            RagWgRed a = it[i];
            a.blk_begin = blocks;
            blocks += (int)((a.n_w + a.n_b + RWG_THREADS - 1) / RWG_THREADS);
            bytes += 4.0 * (double)(a.n_w + a.n_b) * (a.nsplit + 1);
            R.it[R.n++] = a;
        }
        if (blocks == 0) continue;
        ProfScope ps(AVC_K_REDUCE, 0.0, bytes, s);
        hipLaunchKernelGGL(rwg_reduce_kernel, dim3(blocks), dim3(RWG_THREADS), 0, s, R);
        if (int rc = (int)hipGetLastError()) return rc;
    }
    return 0;
}

// ---- op level -------------------------------------------------------------------------------------------------------------------------
// tables of one call, in the order they lie at the head of the caller's workspace (ints): Tin[B] | offin[B + 1] | Tout[B] | offout[B + 1] |
// chunk[2 nchunks], each padded to 4
static long rwg_op_tables(int B, const int* T, int stride, std::vector<int>& tab, long off[5], int* nchunks) {
    tab.clear();
    auto put = [&](const std::vector<int>& v) {
        const long o = (long)tab.size();
        tab.insert(tab.end(), v.begin(), v.end());
        while (tab.size() % 4) tab.push_back(0);
        return o;
    };
    std::vector<int> Ti(T, T + B), oi(B + 1, 0), To(B), oo(B + 1, 0), ch;
    for (int b = 0; b < B; ++b) {
        To[b] = avc_cdiv(T[b], stride);
        oi[b + 1] = oi[b] + Ti[b];
        oo[b + 1] = oo[b] + To[b];
        for (int t0 = 0; t0 < To[b]; t0 += 32) {
            ch.push_back(b);
            ch.push_back(t0);
        }
    }
    off[0] = put(Ti); off[1] = put(oi); off[2] = put(To); off[3] = put(oo); off[4] = put(ch);
    *nchunks = (int)ch.size() / 2;
    return ((long)tab.size() + 63) / 64 * 64;
}

static int rwg_op_check(int B, const int* T, int Cin, int Cout, int KS, int stride) {
    if (B < 1 || !T || Cin < 1 || Cout < 1 || KS < 1 || KS > 8 || stride < 1 || stride > 2) return -1;
    long sum = 0;
    for (int b = 0; b < B; ++b) {
        if (T[b] < 1) return -1;
        if (KS / 2 >= T[b]) return -6;   // the reflect-pad rule, per sample
        sum += T[b];
    }
    return sum * (long)(Cin > Cout ? Cin : Cout) >= (1L << 31) ? -1 : 0;
}

extern "C" long avc_conv1d_wgrad_ragged_ws_floats(int B, const int* T, int Cin, int Cout, int KS, int stride) {
    if (rwg_op_check(B, T, Cin, Cout, KS, stride)) return -1;
    std::vector<int> tab;
    long off[5];
    int nchunks;
    const long head = rwg_op_tables(B, T, stride, tab, off, &nchunks);
    const int ns = avc_rwg_nsplit(Cin, Cout, nchunks);
    return head + (ns > 1 ? (long)ns * avc_rwg_slot_floats(Cin, Cout, KS) : 0);
}

extern "C" int avc_conv1d_wgrad_ragged(const float* x, int xC, int xc0, const float* dy, int dyC, int dyc0, int B, const int* T, int Cin, int Cout,
                                       int KS, int stride, float* dW, float* db, float* ws, void* stream) {
    if (!x || !dy || !dW || !ws) return -1;
    if (int rc = rwg_op_check(B, T, Cin, Cout, KS, stride)) return rc;
    if (xc0 < 0 || dyc0 < 0 || xc0 + Cin > xC || dyc0 + Cout > dyC) return -1;
    hipStream_t s = (hipStream_t)stream;
    static thread_local std::vector<int> tab;   // (outlives the call: the copy below reads it)
    long off[5];
    int nchunks;
    const long head = rwg_op_tables(B, T, stride, tab, off, &nchunks);
    if (int rc = (int)hipMemcpyAsync(ws, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, s)) return rc;
    const int* dt = (const int*)ws;
    RagWgJob j;
    memset(&j, 0, sizeof(j));
    j.x = x; j.dy = dy;
    j.Tin = dt + off[0]; j.offin = dt + off[1]; j.Tout = dt + off[2]; j.offout = dt + off[3]; j.chunk = dt + off[4];
    j.xC = xC; j.xc0 = xc0; j.dyC = dyC; j.dyc0 = dyc0;
    j.Cin = Cin; j.Cout = Cout; j.KS = KS; j.stride = stride;
    j.nchunks = nchunks;
    j.nsplit = avc_rwg_nsplit(Cin, Cout, nchunks);
    j.slot_floats = avc_rwg_slot_floats(Cin, Cout, KS);
    j.out = j.nsplit > 1 ? ws + head : dW;
    j.db = db;
    if (int rc = avc_launch_rwg(&j, 1, s)) return rc;
    if (j.nsplit == 1) return 0;
    RagWgRed r;
    memset(&r, 0, sizeof(r));
    r.slab = j.out; r.dw = dW; r.db = db;
    r.slot_floats = j.slot_floats; r.n_w = (long)Cout * Cin * KS; r.n_b = Cout; r.nsplit = j.nsplit;
    return avc_launch_rwg_reduce(&r, 1, s);
}

// ---- op level: a Linear's weight gradient over N rows read through strides -------------------------------------------------------------
//     dW[co][ci] = sum_n dy(n, co) x(n, ci),   db[co] = sum_n dy(n, co),     x(n, ci) = x[n sxn + ci sxc],   dy(n, co) = dy[n syn + co syc]
// ONE strided job of the kernel above (the N rows are its frames).  The walk is avc_conv1d_wgrad_ragged's at B = 1, T = N, KS = 1: with
// sxn = syn = 1, sxc = syc = N the two give the same bits.
static int rwg_strided_check(long sxn, long sxc, long syn, long syc, int N, int Cin, int Cout) {
    if (N < 1 || Cin < 1 || Cout < 1 || sxn < 0 || sxc < 0 || syn < 0 || syc < 0) return -1;
    if ((N - 1) * sxn + (Cin - 1) * sxc >= (1L << 31) || (N - 1) * syn + (Cout - 1) * syc >= (1L << 31)) return -1;
    return 0;
}

void avc_rwg_strided_job(RagWgJob& j, const float* x, long sxn, long sxc, const float* dy, long syn, long syc, int N, int Cin, int Cout) {
    memset(&j, 0, sizeof(j));
    j.x = x; j.dy = dy;
    j.strided = 1; j.nframes = N;
    j.sxc = sxc; j.sxt = sxn; j.syc = syc; j.syt = syn;
    j.Cin = Cin; j.Cout = Cout; j.KS = 1; j.stride = 1;
    j.nchunks = avc_cdiv(N, 32);
    j.nsplit = avc_rwg_nsplit(Cin, Cout, j.nchunks);
    j.slot_floats = avc_rwg_slot_floats(Cin, Cout, 1);
}

extern "C" long avc_linear_wgrad_strided_ws_floats(int N, int Cin, int Cout) {
    if (N < 1 || Cin < 1 || Cout < 1) return -1;
    const int ns = avc_rwg_nsplit(Cin, Cout, avc_cdiv(N, 32));
    return 64 + (ns > 1 ? (long)ns * avc_rwg_slot_floats(Cin, Cout, 1) : 0);
}

extern "C" int avc_linear_wgrad_strided(const float* x, long sxn, long sxc, const float* dy, long syn, long syc, int N, int Cin, int Cout, float* dW,
                                        float* db, float* ws, void* stream) {
    if (!x || !dy || !dW || !ws) return -1;
    if (int rc = rwg_strided_check(sxn, sxc, syn, syc, N, Cin, Cout)) return rc;
    hipStream_t s = (hipStream_t)stream;
    RagWgJob j;
    avc_rwg_strided_job(j, x, sxn, sxc, dy, syn, syc, N, Cin, Cout);
    j.out = j.nsplit > 1 ? ws + 64 : dW;
    j.db = db;
    if (int rc = avc_launch_rwg(&j, 1, s)) return rc;
    if (j.nsplit == 1) return 0;
    RagWgRed r;
    memset(&r, 0, sizeof(r));
    r.slab = j.out; r.dw = dW; r.db = db;
    r.slot_floats = j.slot_floats; r.n_w = (long)Cout * Cin; r.n_b = Cout; r.nsplit = j.nsplit;
    return avc_launch_rwg_reduce(&r, 1, s);
}
