// The two audio edges for MANY utterances of different lengths in one launch each (dsp.hip has the single-utterance kernels and the
// ragged Griffin-Lim between the edges).  B waveforms lie back to back in one buffer: utterance b is samples woff[b] .. woff[b+1]
// (B + 1 device int64: a corpus chunk can pass 2^31 bytes); frame columns are addressed through B + 1 device int32 offsets as in
// dsp_frames_ragged_kernel.  The entry points (dsp_api.hip) validate the HOST copies of the tables; the kernels index through the
// device copies unchecked.
//
//   dsp_frame_power_ragged_kernel     trim's frame powers: one workgroup per frame, dsp_frame_power_body on the frame's utterance
//   dsp_frames_ragged_preemph_kernel  pre-emphasis fused into the framing of the STFT: no pre-emphasised waveform goes to HBM
//   dsp_deemph_ragged_kernel          the blocked scan of dsp_deemph_body, one workgroup per utterance
//
// Lane layout of the framing kernel: consecutive lanes are consecutive frame columns t of one tap k, as in dsp_frames_kernel.  The
// frames matrix ([win][Ttot], 1200 x Ttot floats at the stock geometry) is what moves: it is written once, 256 contiguous bytes per
// wave.  The reads of a wave are hop samples apart (two neighbouring samples each for the pre-emphasis) and every sample is read by
// win / hop = 4 columns of every tap -- the whole waveform is 1 / win of the frames and stays in L2, so the reads are cache hits and
// staging them through LDS would trade those hits for a layout whose column reads stride the banks by hop (hop = 300: 300 mod 32 = 12,
// a 4-way conflict on ds_read_b32) and for workgroups tied to one utterance each, which leaves a short batch with a grid of a few
// dozen workgroups.  The flat grid-stride form keeps every launch at dsp_blocks() workgroups whatever the lengths are.
#include <hip/hip_runtime.h>

#include "avc_common.h"
#include "avc_internal.h"
#include "dsp_shared.h"

__global__ void __launch_bounds__(AVC_THREADS) dsp_frame_power_ragged_kernel(const float* y, const long* woff, const int* poff, int B, int frame_length,
                                                                              int hop, float* out) {
    __shared__ float red[AVC_THREADS];
    const int b = dsp_find(poff, B, (long)blockIdx.x, 0, false);
    dsp_frame_power_body(y + woff[b], woff[b + 1] - woff[b], frame_length, hop, (long)blockIdx.x - poff[b], red, out + blockIdx.x);
}

// frames[k][toff[b] + t] = pre_b[reflect(t hop + n0 + k - n_fft/2, e_b - s_b)], pre_b = the pre-emphasis of y[woff[b] + s_b .. woff[b] + e_b)
// computed at every read (bounds[2b] = s_b, bounds[2b+1] = e_b)
__global__ void __launch_bounds__(AVC_THREADS) dsp_frames_ragged_preemph_kernel(const float* y, const long* woff, const int* toff, const long* bounds, int B,
                                                                                 int hop, int n_fft, int win, float a, float* frames) {
    const int n0 = (n_fft - win) / 2;
    const long TT = toff[B], total = (long)win * TT;
    for (long e = (long)blockIdx.x * AVC_THREADS + threadIdx.x; e < total; e += (long)gridDim.x * AVC_THREADS) {
        const int k = (int)(e / TT);
        const long c = e - (long)k * TT;
        const int b = dsp_find(toff, B, c, hop, false);
        const long t = c - toff[b];
        const long s = bounds[2 * b], L = bounds[2 * b + 1] - s;
        frames[e] = dsp_preemph_at(y + woff[b] + s, dsp_reflect(t * hop + n0 + k - n_fft / 2, L), a);
    }
}

__global__ void __launch_bounds__(1024) dsp_deemph_ragged_kernel(const float* x, const long* woff, float a, float* out) {
    __shared__ float last[1024], cin[1024], apow[1024];
    const long o = woff[blockIdx.x];
    dsp_deemph_body(x + o, woff[blockIdx.x + 1] - o, a, out + o, last, cin, apow);
}

int avc_launch_dsp_frame_power_ragged(const float* y, const long* woff, const int* poff, int B, int n_frames, int frame_length, int hop, float* out,
                                      hipStream_t s) {
    hipLaunchKernelGGL(dsp_frame_power_ragged_kernel, dim3(n_frames), dim3(AVC_THREADS), 0, s, y, woff, poff, B, frame_length, hop, out);
    return (int)hipGetLastError();
}
int avc_launch_dsp_frames_ragged_preemph(const float* y, const long* woff, const int* toff, const long* bounds, int B, int Ttot, int hop, int n_fft,
                                         int win, float a, float* frames, hipStream_t s) {
    hipLaunchKernelGGL(dsp_frames_ragged_preemph_kernel, dim3(dsp_blocks((long)win * Ttot)), dim3(AVC_THREADS), 0, s, y, woff, toff, bounds, B, hop, n_fft,
                       win, a, frames);
    return (int)hipGetLastError();
}
int avc_launch_dsp_deemph_ragged(const float* x, const long* woff, int B, float a, float* out, hipStream_t s) {
    hipLaunchKernelGGL(dsp_deemph_ragged_kernel, dim3(B), dim3(1024), 0, s, x, woff, a, out);
    return (int)hipGetLastError();
}
