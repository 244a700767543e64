// C-ABI entry points of the mel <-> waveform DSP (declared in include/avc_hip.h; kernels in dsp.hip, the two transforms
// run as 1x1 "convolutions" on conv_gemm.hip's fp32-MFMA kernel).  Reference: preprocess/tacotron/utils.py:27-155.
#include <hip/hip_runtime.h>

#include "avc_common.h"
#include "avc_hip.h"
#include "avc_internal.h"

extern "C" {

int avc_dsp_num_frames(long L, int hop_length) { return (int)(1 + L / hop_length); }   // librosa.stft, center=True

static bool dsp_geom_ok(int n_fft, int hop, int win) { return n_fft >= 4 && (n_fft & 1) == 0 && win >= 2 && win <= n_fft && hop >= 1 && hop <= win; }

long avc_dsp_basis_floats(int n_fft, int win_length, int inverse) {
    const int F2 = n_fft + 2;
    return inverse ? avc_packed_weight_floats(win_length, F2, 1, 0) : avc_packed_weight_floats(F2, win_length, 1, 0);
}
long avc_dsp_basis_scratch_floats(int n_fft, int win_length) { return (long)(n_fft + 2) * win_length; }

int avc_dsp_make_basis(int n_fft, int hop_length, int win_length, int inverse, float* dense_scratch, float* packed, void* stream) {
    if (!dsp_geom_ok(n_fft, hop_length, win_length) || !dense_scratch || !packed) return -1;
    int rc = avc_launch_dsp_basis(inverse ? 1 : 0, n_fft, win_length, dense_scratch, (hipStream_t)stream);
    if (rc) return rc;
    const float* src = dense_scratch;
    const int F2 = n_fft + 2;
    return inverse ? avc_pack_weight(&src, 1, win_length, win_length, F2, 1, 0, packed, stream)
                   : avc_pack_weight(&src, 1, F2, F2, win_length, 1, 0, packed, stream);
}

// spec[2F][B T] = Wf[2F][win] x frames[win][B T]   (B signals of L samples: their frames are columns of one GEMM)
int avc_dsp_stft_batch(const float* y, long L, int B, int n_fft, int hop_length, int win_length, const float* basis_fwd, float* frames_ws,
                       float* spec, void* stream) {
    if (!dsp_geom_ok(n_fft, hop_length, win_length) || !y || !basis_fwd || !frames_ws || !spec || B < 1) return -1;
    if (L <= n_fft / 2) return -6;   // numpy reflect padding needs pad < len (the reference's librosa call raises there)
    const int T = avc_dsp_num_frames(L, hop_length), F2 = n_fft + 2;
    const long BT = (long)B * T;
    if (BT > 0x7fffffffL) return -1;
    int rc = avc_launch_dsp_frames(y, L, B, T, hop_length, n_fft, win_length, frames_ws, (hipStream_t)stream);
    if (rc) return rc;
    return avc_conv1d_fwd(frames_ws, 0, BT, 1, 1, win_length, (int)BT, basis_fwd, nullptr, F2, 1, 1, 0, spec, 0, BT, 1, 1, nullptr, 0, 0, 0,
                          0, 0, nullptr, 0, stream);
}
int avc_dsp_stft(const float* y, long L, int n_fft, int hop_length, int win_length, const float* basis_fwd, float* frames_ws,
                 float* spec, void* stream) {
    return avc_dsp_stft_batch(y, L, 1, n_fft, hop_length, win_length, basis_fwd, frames_ws, spec, stream);
}

// y[hop (T-1)] = overlap-add of tf[win][T] = Wi[win][2F] x spec[2F][T], over the window's sum of squares
int avc_dsp_istft_batch(const float* spec, int B, int T, int n_fft, int hop_length, int win_length, const float* basis_inv, float* tf_ws,
                        float* y, void* stream) {
    if (!dsp_geom_ok(n_fft, hop_length, win_length) || !spec || !basis_inv || !tf_ws || !y || T < 2 || B < 1) return -1;
    const int F2 = n_fft + 2;
    const long BT = (long)B * T;
    if (BT > 0x7fffffffL) return -1;
    int rc = avc_conv1d_fwd(spec, 0, BT, 1, 1, F2, (int)BT, basis_inv, nullptr, win_length, 1, 1, 0, tf_ws, 0, BT, 1, 1, nullptr, 0, 0, 0, 0,
                            0, nullptr, 0, stream);
    if (rc) return rc;
    return avc_launch_dsp_ola(tf_ws, B, T, hop_length, n_fft, win_length, y, (hipStream_t)stream);
}
int avc_dsp_istft(const float* spec, int T, int n_fft, int hop_length, int win_length, const float* basis_inv, float* tf_ws, float* y,
                  void* stream) {
    return avc_dsp_istft_batch(spec, 1, T, n_fft, hop_length, win_length, basis_inv, tf_ws, y, stream);
}

long avc_dsp_griffin_lim_ws_floats(int T, int n_fft, int hop_length, int win_length) {   // T = frames of ALL utterances of a batch
    const long F2 = n_fft + 2;
    auto up = [](long n) { return (n + 63) / 64 * 64; };
    return 2 * up(F2 * T) + up((long)win_length * T) + up((long)hop_length * T);
}

// utils.py:136-147: X = S; repeat n_iter: x = istft(X); est = stft(x); X = S * est / max(1e-8, |est|); return istft(X)
// B utterances of T frames each: S is [F][B T] (utterance b in columns b T .. b T + T - 1), y is [B][hop (T - 1)]
int avc_dsp_griffin_lim_batch(const float* S, int B, int T, int n_fft, int hop_length, int win_length, int n_iter, const float* basis_fwd,
                              const float* basis_inv, float* ws, float* y, void* stream) {
    if (!dsp_geom_ok(n_fft, hop_length, win_length) || !S || !basis_fwd || !basis_inv || !ws || !y || T < 2 || B < 1 || n_iter < 0) return -1;
    const long Ly = (long)hop_length * (T - 1), BT = (long)B * T;
    if (Ly <= n_fft / 2) return -6;
    if (BT > 0x7fffffffL) return -1;
    const int F = n_fft / 2 + 1;
    const long F2 = n_fft + 2;
    auto up = [](long n) { return (n + 63) / 64 * 64; };
    float* xbest = ws;
    float* est = xbest + up(F2 * BT);
    float* fr = est + up(F2 * BT);                 // frames of the STFT / time frames of the iSTFT (never live together)
    float* xt = fr + up((long)win_length * BT);
    hipStream_t s = (hipStream_t)stream;
    int rc = avc_launch_dsp_phase(nullptr, S, F, (int)BT, xbest, s);
    for (int i = 0; i < n_iter && !rc; ++i) {
        rc = avc_dsp_istft_batch(xbest, B, T, n_fft, hop_length, win_length, basis_inv, fr, xt, stream);
        if (!rc) rc = avc_dsp_stft_batch(xt, Ly, B, n_fft, hop_length, win_length, basis_fwd, fr, est, stream);   // 1 + Ly / hop == T frames
        if (!rc) rc = avc_launch_dsp_phase(est, S, F, (int)BT, xbest, s);
    }
    if (!rc) rc = avc_dsp_istft_batch(xbest, B, T, n_fft, hop_length, win_length, basis_inv, fr, y, stream);
    return rc;
}
int avc_dsp_griffin_lim(const float* S, int T, int n_fft, int hop_length, int win_length, int n_iter, const float* basis_fwd,
                        const float* basis_inv, float* ws, float* y, void* stream) {
    return avc_dsp_griffin_lim_batch(S, 1, T, n_fft, hop_length, win_length, n_iter, basis_fwd, basis_inv, ws, y, stream);
}

// Utterances of DIFFERENT lengths: S is [F][Ttot] with utterance b in columns toff[b] .. toff[b+1]-1 (toff: B + 1 device ints,
// toff[0] = 0, toff[B] = Ttot), y receives the waveforms back to back: utterance b at sample hop (toff[b] - b).  toff_host is the
// HOST copy of the same B + 1 offsets: the kernels index frames and samples through the device array without bounds checks, so the
// library validates the host copy (monotone, toff[0] = 0, toff[B] = Ttot, hop (T_b - 1) > n_fft / 2 for the reflect padding of every
// utterance's STFT: -6, as the equal-length entry point) and the caller keeps the two identical.
int avc_dsp_griffin_lim_ragged(const float* S, const int* toff, const int* toff_host, int B, int Ttot, int n_fft, int hop_length, int win_length,
                               int n_iter, const float* basis_fwd, const float* basis_inv, float* ws, float* y, void* stream) {
    if (!dsp_geom_ok(n_fft, hop_length, win_length) || !S || !toff || !toff_host || !basis_fwd || !basis_inv || !ws || !y || B < 1 || Ttot < 2 * B ||
        n_iter < 0)
        return -1;
    if (toff_host[0] != 0 || toff_host[B] != Ttot) return -1;
    for (int b = 0; b < B; ++b) {
        const int Tb = toff_host[b + 1] - toff_host[b];
        if (Tb < 2) return -1;
        if ((long)hop_length * (Tb - 1) <= n_fft / 2) return -6;
    }
    const int F = n_fft / 2 + 1, F2 = n_fft + 2;
    auto up = [](long n) { return (n + 63) / 64 * 64; };
    float* xbest = ws;
    float* est = xbest + up((long)F2 * Ttot);
    float* fr = est + up((long)F2 * Ttot);
    float* xt = fr + up((long)win_length * Ttot);
    hipStream_t s = (hipStream_t)stream;
    auto istft = [&](const float* spec, float* out) {
        int rc = avc_conv1d_fwd(spec, 0, Ttot, 1, 1, F2, Ttot, basis_inv, nullptr, win_length, 1, 1, 0, fr, 0, Ttot, 1, 1, nullptr, 0, 0, 0, 0, 0,
                                nullptr, 0, stream);
        return rc ? rc : avc_launch_dsp_ola_ragged(fr, toff, B, Ttot, hop_length, n_fft, win_length, out, s);
    };
    int rc = avc_launch_dsp_phase(nullptr, S, F, Ttot, xbest, s);
    for (int i = 0; i < n_iter && !rc; ++i) {
        rc = istft(xbest, xt);
        if (!rc) rc = avc_launch_dsp_frames_ragged(xt, toff, B, Ttot, hop_length, n_fft, win_length, fr, s);
        if (!rc) rc = avc_conv1d_fwd(fr, 0, Ttot, 1, 1, win_length, Ttot, basis_fwd, nullptr, F2, 1, 1, 0, est, 0, Ttot, 1, 1, nullptr, 0, 0, 0, 0, 0,
                                     nullptr, 0, stream);
        if (!rc) rc = avc_launch_dsp_phase(est, S, F, Ttot, xbest, s);
    }
    if (!rc) rc = istft(xbest, y);
    return rc;
}

int avc_dsp_magnitude(const float* spec, int n_fft, int T, float* mag, void* stream) {
    if (!spec || !mag || T < 1) return -1;
    return avc_launch_dsp_mag(spec, n_fft / 2 + 1, T, mag, (hipStream_t)stream);
}
int avc_dsp_db_normalize(const float* in, int C, int T, float ref_db, float max_db, float* out, void* stream) {
    if (!in || !out || C < 1 || T < 1) return -1;
    return avc_launch_dsp_db_norm(in, C, T, ref_db, max_db, out, (hipStream_t)stream);
}
int avc_dsp_denormalize_amp(const float* in, int C, int T, float ref_db, float max_db, float* out, void* stream) {
    if (!in || !out || C < 1 || T < 1) return -1;
    return avc_launch_dsp_denorm_amp(in, C, T, ref_db, max_db, out, (hipStream_t)stream);
}
int avc_dsp_preemphasis(const float* y, long L, float a, float* out, void* stream) {
    if (!y || !out || L < 1 || y == out) return -1;
    return avc_launch_dsp_preemph(y, L, a, out, (hipStream_t)stream);
}
int avc_dsp_deemphasis(const float* x, long L, float a, float* out, void* stream) {
    if (!x || !out || L < 1) return -1;
    return avc_launch_dsp_deemph(x, L, a, out, (hipStream_t)stream);
}
int avc_dsp_frame_power(const float* y, long L, int frame_length, int hop_length, float* out, void* stream) {
    if (!y || !out || frame_length < 2 || hop_length < 1) return -1;
    if (L <= frame_length / 2) return -6;
    // 1 + (L + 2 (frame_length / 2) - frame_length) / hop frames fit the padded signal: an ODD frame_length pads one sample less than it
    // spans, and counting 1 + L / hop would cut a last frame that reaches one sample past the padding (index -1 at L = frame_length/2 + 1)
    return avc_launch_dsp_frame_power(y, L, frame_length, hop_length, avc_dsp_num_frames(L - (frame_length & 1), hop_length), out, (hipStream_t)stream);
}

// ---- B utterances of different lengths, packed back to back: utterance b is samples woff[b] .. woff[b+1] of one buffer (B + 1 int64,
// woff[0] = 0, every utterance at least one sample).  Every table comes twice, as for avc_dsp_griffin_lim_ragged: the device copy the
// kernels index through, and the HOST copy that is validated here -- a refused call launches nothing.
static bool dsp_woff_ok(const long* woff_host, int B) {
    if (woff_host[0] != 0) return false;
    for (int b = 0; b < B; ++b)
        if (woff_host[b + 1] <= woff_host[b]) return false;
    return true;
}

// avc_dsp_frame_power of every utterance in ONE launch: the powers of utterance b go to out[poff[b] .. poff[b+1]), poff[b+1] - poff[b] =
// 1 + (L_b - frame_length % 2) / hop, the count of the single entry point (poff: B + 1 int32 from 0)
int avc_dsp_frame_power_ragged(const float* y, const long* woff, const long* woff_host, const int* poff, const int* poff_host, int B,
                               int frame_length, int hop_length, float* out, void* stream) {
    if (!y || !woff || !woff_host || !poff || !poff_host || !out || B < 1 || frame_length < 2 || hop_length < 1) return -1;
    if (!dsp_woff_ok(woff_host, B) || poff_host[0] != 0) return -1;
    for (int b = 0; b < B; ++b)
        if (woff_host[b + 1] - woff_host[b] <= frame_length / 2) return -6;
    for (int b = 0; b < B; ++b) {
        const long nf = 1 + (woff_host[b + 1] - woff_host[b] - (frame_length & 1)) / hop_length;
        if (nf > 0x7fffffffL - poff_host[b] || poff_host[b + 1] != poff_host[b] + (int)nf) return -1;
    }
    return avc_launch_dsp_frame_power_ragged(y, woff, poff, B, poff_host[B], frame_length, hop_length, out, (hipStream_t)stream);
}

// Pre-emphasis (utils.py:60) fused into the framing of librosa.stft (utils.py:63-66) for B utterances: utterance b is the sub-run
// [woff[b] + s_b, woff[b] + e_b) of the packed buffer, (s_b, e_b) = bounds[2b], bounds[2b+1] (2B int64: what trim chose, or 0 and L_b); its
// T_b = 1 + (e_b - s_b) / hop frames are columns toff[b] .. toff[b+1] - 1 of frames [win_length][Ttot], reflect-padded at the TRIMMED length.
// -6 when an utterance has e_b - s_b <= n_fft / 2, -1 when toff disagrees with the bounds.  The STFT is avc_conv1d_fwd on frames.
int avc_dsp_frames_ragged_preemph(const float* y, const long* woff, const long* woff_host, const int* toff, const int* toff_host, const long* bounds,
                                  const long* bounds_host, int B, int n_fft, int hop_length, int win_length, float a, float* frames, void* stream) {
    if (!dsp_geom_ok(n_fft, hop_length, win_length) || !y || !woff || !woff_host || !toff || !toff_host || !bounds || !bounds_host || !frames || B < 1)
        return -1;
    if (!dsp_woff_ok(woff_host, B) || toff_host[0] != 0) return -1;
    for (int b = 0; b < B; ++b) {
        const long s = bounds_host[2 * b], e = bounds_host[2 * b + 1];
        if (s < 0 || e < s || e > woff_host[b + 1] - woff_host[b]) return -1;
    }
    for (int b = 0; b < B; ++b)
        if (bounds_host[2 * b + 1] - bounds_host[2 * b] <= n_fft / 2) return -6;
    for (int b = 0; b < B; ++b) {
        const long Tb = 1 + (bounds_host[2 * b + 1] - bounds_host[2 * b]) / hop_length;
        if (Tb > 0x7fffffffL - toff_host[b] || toff_host[b + 1] != toff_host[b] + (int)Tb) return -1;
    }
    return avc_launch_dsp_frames_ragged_preemph(y, woff, toff, bounds, B, toff_host[B], hop_length, n_fft, win_length, a, frames, (hipStream_t)stream);
}

// avc_dsp_deemphasis of every utterance in ONE launch, one workgroup each (x == out is allowed, as there)
int avc_dsp_deemphasis_ragged(const float* x, const long* woff, const long* woff_host, int B, float a, float* out, void* stream) {
    if (!x || !woff || !woff_host || !out || B < 1 || !dsp_woff_ok(woff_host, B)) return -1;
    return avc_launch_dsp_deemph_ragged(x, woff, B, a, out, (hipStream_t)stream);
}
}
