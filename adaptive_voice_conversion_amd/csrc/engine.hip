// Whole-model orchestration of the AdaIN-VC autoencoder on gfx950: builds the
// launch plan for one (B, T, T_cond) shape and issues the forward / backward
// kernel sequences on the caller's stream.
//
// Reference being replaced (never copied): AE.forward / AE.inference
// (model.py:380-391), SpeakerEncoder.forward (:265-277), ContentEncoder.forward
// (:301-323), Decoder.forward (:347-371) and their autograd; the loss of
// solver.py:84-88.  Parameter order = state_dict registration order.
//
// HBM layout: one caller-owned fp32 workspace.  Packed weights, every saved
// activation ([B,C,T], T contiguous), IN statistics, gradient temporaries and
// the split-K slabs of the weight gradients live at fixed offsets decided at
// plan creation; nothing is allocated, freed or synchronised here.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "avc_common.h"
#include "avc_hip.h"
#include "avc_internal.h"

static thread_local std::string g_err;
static int fail(int rc, const char* what) {
    char buf[256];
    snprintf(buf, sizeof(buf), "%s (rc=%d)", what, rc);
    g_err = buf;
    return rc;
}
#define RUN(expr)                                  \
    do {                                           \
        int _rc = (expr);                          \
        if (_rc != 0) return fail(_rc, #expr);     \
    } while (0)

// messages that differ between entry points by the function name only
static int fail(int rc, const char* fn, const char* what) { return fail(rc, (std::string(fn) + ": " + what).c_str()); }
// a caller's [rows][cols] matrix with element strides seb / sec (the conv kernel addresses its source with 32-bit element offsets; -1
// marks a structural zero)
static int check_row_strides(const char* fn, const char* what, long rows, long cols, long seb, long sec) {
    if (seb < 0 || sec < 0 || (rows - 1) * seb + (cols - 1) * sec >= (1L << 31))
        return fail(-1, fn, (std::string(what) + " strides must be non-negative and span less than 2^31 elements").c_str());
    return 0;
}

extern "C" const char* avc_last_error(void) { return g_err.c_str(); }
extern "C" int avc_version(void) { return 100; }


struct ParamT {
    long off, numel;
    int d[3];
};

struct LayerP {
    int bf16 = 0;  // AVC_COMPUTE_* of this layer's matrix products (avc_plan_set_compute_dtype)
    int Cout = 0, Cin = 0, KS = 1, stride = 1;
    int nsrc = 1, rows = 0;
    int w[12], b[12];
    long wpf = -1, wpd = -1, bpk = -1;
    int CK = 8, CKd = 8, nchunk_f = 0, nchunk_d = 0, Mp_f = 0, Mp_d = 0, dgM = 0;
    bool need_dgrad = true;
    bool x3_f = false, x3_d = false;   // split-bf16 kernel (conv_x3.hip): image at wrs_f / wrs_d, 16-channel chunks
    long wrs_f = -1, wrs_d = -1;
    bool conv_path = true;             // launched through conv_gemm.hip (AVC_IMG_K4 images); false: the dense stack (AVC_IMG_PLAIN)
    long wplain = -1;                  // extra AVC_IMG_PLAIN forward image (the affine layer: its d_emb GEMM reads it as a [Kp][Mp] matrix)
    bool bh = false;                   // bf16 pair operands (AVC_PLAN_BF16S): AVC_IMG_K4H images over Cin / 2 (Cout / 2) dword channels
    long src_off = 0;                  // input-gradient image of input rows [src_off, src_off + dgM) of w[0] only (the in_conv's pass-through rows)
    int rwg_nsplit = 1;                // ragged plans with AVC_PLAN_PART_GRADS: split-K ways of this layer's ragged weight gradient, and its
    long rwg_slab = -1;                // slots (a stacked layer: one set of slots per source tensor, back to back)
};

struct EncNet {
    avc_encoder_cfg c;
    float slope = 0.f;   // activation slope of this network (0 = ReLU, AVC_LRELU_SLOPE = 'lrelu')
    int nb = 0, CC = 0, n = 0, nd = 0;
    int T[AVC_MAX_BLOCKS + 1];
    std::vector<int> bank, c1, c2, dn1, dn2;
    int in_conv = -1, outl = -1, heads = -1;
    int in_pass = -1;                               // AVC_PLAN_INPUT_GRADS: input-gradient image of the in_conv's M pass-through rows
    long dx = -1;                                   // AVC_PLAN_INPUT_GRADS: d(loss)/d(x) [B, M, T0] fp32
    long cat = -1, dcat = -1, h0 = -1;              // h0: speaker relu(in_conv) / content y0
    long out[AVC_MAX_BLOCKS + 1];                   // block outputs (out[0] = after in_conv stage)
    long a1[AVC_MAX_BLOCKS], a2[AVC_MAX_BLOCKS];    // speaker: relu outputs; content: a1 = relu(IN(y1))
    long y1[AVC_MAX_BLOCKS], y2[AVC_MAX_BLOCKS];    // content conv outputs (pre-norm)
    long st0 = -1, st1[AVC_MAX_BLOCKS], st2[AVC_MAX_BLOCKS];  // IN stats: mean at off, rstd at off + B*C
    long pooled = -1, d1[AVC_MAX_BLOCKS], d2[AVC_MAX_BLOCKS], hd[AVC_MAX_BLOCKS + 1];
};

struct DecNet {
    avc_decoder_cfg c;
    float slope = 0.f;
    int n = 0;
    int T[AVC_MAX_BLOCKS + 1];
    std::vector<int> c1, c2;
    int in_conv = -1, affine = -1, out_conv = -1;
    long z = -1, cond = -1, dcond = -1, y0 = -1;
    long out[AVC_MAX_BLOCKS + 1], y1[AVC_MAX_BLOCKS], a1[AVC_MAX_BLOCKS], y2[AVC_MAX_BLOCKS];
    long st0 = -1, st1[AVC_MAX_BLOCKS], st2[AVC_MAX_BLOCKS];
};

struct avc_plan {
    avc_model_cfg cfg;
    int B, T, Tc, M, Tb, Tout;
    std::vector<ParamT> params;
    long param_floats = 0;
    std::vector<LayerP> layers;
    EncNet spk, enc;
    DecNet dec;
    long ws_top = 0;
    std::map<std::string, long> named;
    // shared gradient temporaries
    long gA = -1, gB = -1, gC = -1;
    long muls = -1, dmuls = -1, emb = -1, demb = -1, decb = -1, ddec = -1, dz = -1;
    long losses = -1, loss_partial = -1;
    long slab = -1, slab_floats = 0;
    long dhA = -1;
    std::vector<avc_relu_site> sites;
    // second gradient-temporary set + side stream: the speaker and content encoders are independent
    // branches (model.py:381-382) and run concurrently so that their small-T layers fill the chip
    long gA2 = -1, gB2 = -1, gC2 = -1;
    mutable hipStream_t side = nullptr;
    mutable hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int compute = 0;             // AVC_COMPUTE_*
    mutable int side_state = 0;  // 0 = not created, 1 = ready, -1 = disabled
    // weight-gradient kernels depend on nothing downstream: they run on their own (low priority)
    // streams beside the dgrad / InstanceNorm-backward chain of each branch
    mutable hipStream_t wstream[2] = {nullptr, nullptr};
    mutable std::vector<hipEvent_t> wev;   // sized by the dry run of the backward pass (one per ordering edge)
    mutable hipEvent_t wjoin[2] = {nullptr, nullptr};
    mutable hipEvent_t ev_dense = nullptr;       // recorded behind the dense-stack backward kernel (the decoder's weight gradients wait for it)
    mutable hipEvent_t ev_dec_grads = nullptr;   // recorded when the decoder's parameter gradients are final
    mutable hipEvent_t ev_spk_grads = nullptr;   // ... the speaker encoder's
    mutable hipEvent_t ev_all_grads = nullptr;   // recorded at the end of avc_backward
    long dyarena = -1, dyarena_floats = 0;
    int flags = 0;            // AVC_PLAN_*
    // ragged inference plans (avc_plan_create_ragged): per-level length / offset / tile tables
    struct RagLevel {
        std::vector<int> T, off;   // per-sample frames, prefix sums (B + 1 entries)
        int ntiles = 0;
        long dT = -1, doff = -1, dtile = -1;   // workspace offsets (in floats == ints) of the device copies
        long dchunk = -1;                      // avc_plan_create_ragged_speaker_grads: the weight gradient's K-chunks, (sample, first frame)
        int nchunks = 0;                       // per 32 frames of one sample
    };
    std::vector<RagLevel> rl_spk, rl_enc, rl_dec;   // speaker / content encoder levels 0..n, decoder levels 0..n (rl_dec[0] == rl_enc[n])
    // fan-out plans (avc_plan_create_ragged_fanout): the decoder has a sample count of its own.  rl_z: the B SOURCES' latent level (the
    // content encoder's last level, or the caller's latent lengths); rl_map: T / off of every OUTPUT's source in rl_z (Nd entries, no
    // tiles: off is a gather, not a prefix sum); rl_dec: the Nd outputs.  Every other ragged plan: Nd == B, both are rl_dec[0].
    int Nd = 0;
    RagLevel rl_z, rl_map;
    // avc_plan_create_ragged_speaker_grads: the dense stack's [C][B] rows as ONE sample of B frames (the Linears' weight gradients run on
    // the ragged kernel too), and one d(pre-activation) row set per dense layer
    RagLevel rl_dense;
    std::vector<long> rag_dz;
    // avc_plan_create_ragged_content_param_grads / _decoder_param_grads: one more set of gradient rows -- conv1's dy of a block, so that it
    // does not overwrite conv2's (gA) before the block's one weight-gradient launch has read both
    long rag_dy1 = -1;
    std::vector<int> rag_host;                     // host image of all tables (uploaded by avc_forward_ragged)
    long rag_tab = -1;
    avc_tuning tun;           // launch heuristics / diagnostic switches, captured at plan creation (the dry run sizes slabs and events with them)
    int nev_need = 0;         // events one backward pass records on the wgrad streams
    long dec_param_off = 0;   // first float of the decoder's parameters in the flat buffer (they are the tail)
    long enc_param_off = 0;   // first float of the content encoder's (the speaker encoder's are the head)
    // AVC_PLAN_BF16S: every [B, C, T] activation / activation gradient is a bf16 pair tensor (bf16_pairs.h) at the same workspace
    // offsets (half of each allocation is used); muls / dec / emb / cond and their gradients, statistics, slabs stay fp32
    // every weight image of the plan as ONE launch (avc_plan_pack_weights / the head of avc_forward): descriptor table in device memory,
    // pointers stored as byte offsets from the caller's parameter buffer / workspace.  Built at plan creation, owned by the plan.
    mutable PackArgs* pack_tab_dev = nullptr;
    mutable void* pack_blk_dev = nullptr;   // (image, piece) of every block of the launch
    int pack_nblk = 0, pack_nblk_early = 0, pack_early_imgs = 0;   // blocks [0, pack_nblk_early) pack the images the step's first kernels read
    double pack_tab_bytes = 0;
    bool bh = false;
    long ddecp = -1, dmulsp = -1;   // pair copies of d(dec) and d(muls): the conv launches that consume them read pair operands
    long demb_rm = -1;              // decoder part plans: d(emb) row-major [B, c_cond] (ws["d_emb"]; demb stays the GEMM's channel-major output)

    long alloc(long n) {
        long o = ws_top;
        ws_top += (n + 63) / 64 * 64;
        return o;
    }
    const float* par(const float* params_, int idx) const { return params_ + params[idx].off; }
};

#define AVC_PLAN_PARTS (AVC_PLAN_SPEAKER_ONLY | AVC_PLAN_CONTENT_ONLY | AVC_PLAN_DECODER_ONLY)
// which of the three networks a plan runs (part plans: one of them)
static bool has_spk(int flags) { return !(flags & (AVC_PLAN_CONTENT_ONLY | AVC_PLAN_DECODER_ONLY)); }
static bool has_enc(int flags) { return !(flags & (AVC_PLAN_SPEAKER_ONLY | AVC_PLAN_DECODER_ONLY)); }
static bool has_dec(int flags) { return !(flags & (AVC_PLAN_SPEAKER_ONLY | AVC_PLAN_CONTENT_ONLY)); }
// (ragged plans: has_enc / has_dec as above; the speaker encoder stays out wherever the caller brings the embeddings, AVC_PLAN_EMB_INPUT,
// which every ragged plan with AVC_PLAN_DECODER_ONLY carries)
static bool rag_has_spk(int flags) { return !(flags & (AVC_PLAN_EMB_INPUT | AVC_PLAN_CONTENT_ONLY)); }

// --------------------------------------------------------------------------
// plan construction
// --------------------------------------------------------------------------
static int add_param(avc_plan* p, int d0, int d1, int d2) {
    ParamT t;
    t.d[0] = d0;
    t.d[1] = d1;
    t.d[2] = d2;
    t.numel = (long)d0 * (d1 > 0 ? d1 : 1) * (d2 > 0 ? d2 : 1);
    t.off = p->param_floats;
    p->param_floats += (t.numel + 3) / 4 * 4;
    p->params.push_back(t);
    return (int)p->params.size() - 1;
}

static int add_layer(avc_plan* p, int Cout, int Cin, int KS, int stride, bool conv3d) {
    LayerP L;
    L.Cout = Cout;
    L.Cin = Cin;
    L.KS = KS;
    L.stride = stride;
    L.nsrc = 1;
    L.rows = Cout;
    L.w[0] = add_param(p, Cout, Cin, conv3d ? KS : 0);
    L.b[0] = add_param(p, Cout, 0, 0);
    p->layers.push_back(L);
    return (int)p->layers.size() - 1;
}

// Bn/Tf: batch and output length of the forward launch; Td: output length of the dgrad launch
// conv_path: the layer is launched through avc_launch_conv (false: the dense stack, which reads plain fp32 images in its own kernel)
static void finish_layer(avc_plan* p, LayerP& L, bool need_dgrad, int dgM, int Bn, int Tf, int Td, int ngroups = 1, bool conv_path = true,
                         bool pairs_ok = true) {
    const avc_tuning& tun = p->tun;
    L.conv_path = conv_path;
    L.bh = p->bh && conv_path && pairs_ok;
    if (p->bh) L.bf16 = L.bh ? AVC_COMPUTE_BF16S : AVC_COMPUTE_BF16;   // (fp32-stored operands of the affine / dense layers: rounded on the way in)
    L.Mp_f = avc_cdiv(L.Cout, 128) * 128;
    L.need_dgrad = need_dgrad;
    L.dgM = dgM > 0 ? dgM : L.Cin;
    L.Mp_d = avc_cdiv(L.dgM, 128) * 128;
    int tf = avc_conv_pick_tile(tun, L.Mp_f, Bn, Tf, ngroups, L.Cin * L.KS);
    L.CK = avc_conv_ck_for(tun, L.KS, avc_conv_num_wgs(tf, L.Mp_f, Bn, Tf, ngroups), 0, L.stride, Tf, tf);
    int td = avc_conv_pick_tile(tun, L.Mp_d, Bn, Td, 1, L.Cout * L.KS);
    L.CKd = avc_conv_ck_for(tun, L.KS, avc_conv_num_wgs(td, L.Mp_d, Bn, Td, 1), 1, L.stride, Td, td);
    if (L.bh && L.KS >= 4 && ngroups == 1) {   // chunk depth in dword channels (tuning bh_ck5; measured: 8 beats 16 beats 32 on the step)
        const int want = (tun.bh_ck5 == 16 || tun.bh_ck5 == 32) ? (int)tun.bh_ck5 : 8;
        L.CK = want;
        L.CKd = want;
    }
    L.nchunk_f = avc_cdiv(L.bh ? L.Cin / 2 : L.Cin, L.CK);
    L.nchunk_d = avc_cdiv(L.bh ? L.Cout / 2 : L.Cout, L.CKd);
    L.x3_f = !p->bh && conv_path && ngroups == 1 && L.nsrc == 1 && avc_conv_x3_eligible(tun, 0, L.Cin, L.KS, L.stride, Tf, Bn, L.Cout);
    L.x3_d = !p->bh && conv_path && need_dgrad && ngroups == 1 && L.nsrc == 1 && avc_conv_x3_eligible(tun, 1, L.Cout, L.KS, L.stride, Td, Bn, L.dgM);
    if (L.x3_f) { L.CK = L.KS == 1 ? 32 : 16; L.nchunk_f = avc_cdiv(L.Cin, L.CK); }
    if (L.x3_d) { L.CKd = L.KS == 1 ? 32 : 16; L.nchunk_d = avc_cdiv(L.Cout, L.CKd); }
    if (L.x3_f) L.wrs_f = p->alloc(avc_conv_x3_image_floats(L.Cout, L.Cin, L.KS));
    if (L.x3_d) L.wrs_d = p->alloc(avc_conv_x3_image_floats(L.dgM, L.Cout, L.KS));
    L.wpf = p->alloc((long)L.nchunk_f * L.KS * L.CK * L.Mp_f);
    if (need_dgrad) L.wpd = p->alloc((long)L.nchunk_d * L.KS * L.CKd * L.Mp_d);
    if (L.nsrc > 1) L.bpk = p->alloc((long)32 * L.Mp_f);
}

static int validate_enc(const avc_encoder_cfg& c, bool spk) {
    if (c.c_in < 1 || c.c_h < 1 || c.c_out < 1 || c.c_bank < 1) return -1;
    if (c.kernel_size < 1 || c.kernel_size > 8) return -1;
    if (c.act != 0 && c.act != 1) return -1;
    if (c.bank_scale < 1 || c.bank_size < c.bank_scale || c.bank_size > 8) return -1;
    if (c.bank_size / c.bank_scale > AVC_MAX_GROUPS) return -1;
    if (c.n_conv_blocks < 1 || c.n_conv_blocks > AVC_MAX_BLOCKS) return -1;
    if (spk && (c.n_dense_blocks < 0 || c.n_dense_blocks > AVC_MAX_BLOCKS)) return -1;
    for (int l = 0; l < c.n_conv_blocks; ++l)
        if (c.subsample[l] != 1 && c.subsample[l] != 2) return -1;
    return 0;
}

static void build_enc_params(avc_plan* p, EncNet& e, const avc_encoder_cfg& c, bool spk) {
    e.c = c;
    e.slope = c.act == 1 ? AVC_LRELU_SLOPE : 0.f;
    e.n = c.n_conv_blocks;
    e.nd = spk ? c.n_dense_blocks : 0;
    for (int k = c.bank_scale; k <= c.bank_size; k += c.bank_scale) e.bank.push_back(add_layer(p, c.c_bank, c.c_in, k, 1, true));
    e.nb = (int)e.bank.size();
    e.CC = c.c_bank * (c.bank_size / c.bank_scale) + c.c_in;
    e.in_conv = add_layer(p, c.c_h, e.CC, 1, 1, true);
    for (int l = 0; l < e.n; ++l) e.c1.push_back(add_layer(p, c.c_h, c.c_h, c.kernel_size, 1, true));
    for (int l = 0; l < e.n; ++l) e.c2.push_back(add_layer(p, c.c_h, c.c_h, c.kernel_size, c.subsample[l], true));
    if (spk) {
        for (int l = 0; l < e.nd; ++l) e.dn1.push_back(add_layer(p, c.c_h, c.c_h, 1, 1, false));
        for (int l = 0; l < e.nd; ++l) e.dn2.push_back(add_layer(p, c.c_h, c.c_h, 1, 1, false));
        e.outl = add_layer(p, c.c_out, c.c_h, 1, 1, false);
    } else {
        // mean_layer + std_layer stacked into one 2*c_out head (model.py:297-298,321-322)
        int mean = add_layer(p, c.c_out, c.c_h, 1, 1, true);
        LayerP& L = p->layers[mean];
        int wi = add_param(p, c.c_out, c.c_h, 1), bi = add_param(p, c.c_out, 0, 0);
        L.nsrc = 2;
        L.rows = c.c_out;
        L.Cout = 2 * c.c_out;
        L.w[1] = wi;
        L.b[1] = bi;
        e.heads = mean;
    }
}

// what every plan asks of the three networks' configurations; prefix: the entry point the message names
static int check_model_cfg(const avc_model_cfg& cfg, const char* prefix) {
    if (validate_enc(cfg.spk, true) || validate_enc(cfg.enc, false)) return fail(-2, prefix, "unsupported encoder config");
    const avc_decoder_cfg& dc = cfg.dec;
    if (dc.n_conv_blocks < 1 || dc.n_conv_blocks > AVC_MAX_BLOCKS || 2 * dc.n_conv_blocks > 12 || dc.kernel_size < 1 || dc.kernel_size > 8)
        return fail(-2, prefix, "unsupported decoder config");
    for (int l = 0; l < dc.n_conv_blocks; ++l)
        if (dc.upsample[l] != 1 && dc.upsample[l] != 2) return fail(-2, prefix, "upsample must be 1 or 2");
    if (cfg.spk.c_in != cfg.enc.c_in || cfg.enc.c_in != dc.c_out || dc.c_in != cfg.enc.c_out || dc.c_cond != cfg.spk.c_out)
        return fail(-2, prefix, "inconsistent channel sizes between the three networks");
    return 0;
}

// the decoder's parameters (p->cfg.dec), the tail of the flat buffer: in_conv, the blocks' convs, the 2n affine Linears as one layer, out_conv
static void build_dec_params(avc_plan* p) {
    const avc_decoder_cfg& dc = p->cfg.dec;
    DecNet& d = p->dec;
    d.c = dc;
    d.slope = dc.act == 1 ? AVC_LRELU_SLOPE : 0.f;
    d.n = dc.n_conv_blocks;
    p->dec_param_off = p->param_floats;
    d.in_conv = add_layer(p, dc.c_h, dc.c_in, 1, 1, true);
    for (int l = 0; l < d.n; ++l) d.c1.push_back(add_layer(p, dc.c_h, dc.c_h, dc.kernel_size, 1, true));
    for (int l = 0; l < d.n; ++l) d.c2.push_back(add_layer(p, dc.c_h * dc.upsample[l], dc.c_h, dc.kernel_size, 1, true));
    const int a0 = add_layer(p, 2 * dc.c_h, dc.c_cond, 1, 1, false);
    LayerP& L = p->layers[a0];
    L.nsrc = 2 * d.n;
    L.rows = 2 * dc.c_h;
    L.Cout = 2 * dc.c_h * L.nsrc;
    for (int i = 1; i < L.nsrc; ++i) {
        L.w[i] = add_param(p, 2 * dc.c_h, dc.c_cond, 0);
        L.b[i] = add_param(p, 2 * dc.c_h, 0, 0);
    }
    d.affine = a0;
    d.out_conv = add_layer(p, dc.c_out, dc.c_h, 1, 1, true);
}

static void plan_init_streams(avc_plan* p);

extern "C" int avc_plan_create(const avc_model_cfg* cfg, int B, int T, int T_cond, avc_plan** out) {
    return avc_plan_create_ex(cfg, B, T, T_cond, 0, out);
}

extern "C" int avc_plan_create_ex(const avc_model_cfg* cfg, int B, int T, int T_cond, int flags, avc_plan** out) {
    return avc_plan_create_tuned(cfg, B, T, T_cond, flags, nullptr, out);
}

extern "C" int avc_plan_create_tuned(const avc_model_cfg* cfg, int B, int T, int T_cond, int flags, const avc_tuning* tuning, avc_plan** out) {
    if (!cfg || !out || B < 1 || T < 1) return fail(-1, "avc_plan_create: bad arguments");
    if (flags & ~(AVC_PLAN_INFERENCE | AVC_PLAN_PARTS | AVC_PLAN_PART_GRADS | AVC_PLAN_X3 | AVC_PLAN_BF16S | AVC_PLAN_INPUT_GRADS)) return fail(-1, "avc_plan_create: unknown flag");
    if ((flags & AVC_PLAN_X3) && (flags & AVC_PLAN_BF16S)) return fail(-1, "avc_plan_create: AVC_PLAN_X3 and AVC_PLAN_BF16S exclude each other");
    if (tuning && tuning->struct_size != (int)sizeof(avc_tuning)) return fail(-1, "avc_plan_create_tuned: avc_tuning of another library version (use avc_tuning_init)");
    const int part = flags & AVC_PLAN_PARTS;
    if (part & (part - 1)) return fail(-1, "avc_plan_create: at most one of AVC_PLAN_SPEAKER_ONLY / _CONTENT_ONLY / _DECODER_ONLY");
    if ((flags & AVC_PLAN_PART_GRADS) && !part) return fail(-1, "avc_plan_create: AVC_PLAN_PART_GRADS needs a part flag (whole plans have gradient buffers unless AVC_PLAN_INFERENCE)");
    if ((flags & AVC_PLAN_PART_GRADS) && (flags & AVC_PLAN_INFERENCE)) return fail(-1, "avc_plan_create: AVC_PLAN_PART_GRADS and AVC_PLAN_INFERENCE exclude each other");
    if (part && !(flags & AVC_PLAN_PART_GRADS)) flags |= AVC_PLAN_INFERENCE;   // a part plan is forward-only unless asked for its gradients
    if ((flags & AVC_PLAN_INPUT_GRADS) && (flags & (AVC_PLAN_INFERENCE | AVC_PLAN_DECODER_ONLY)))
        return fail(-1, "avc_plan_create: AVC_PLAN_INPUT_GRADS needs a plan with a backward pass through an encoder (not INFERENCE, not DECODER_ONLY, part plans need PART_GRADS)");
    if (T_cond <= 0) T_cond = T;
    const bool infer = (flags & AVC_PLAN_INFERENCE) != 0;
    const bool ig = (flags & AVC_PLAN_INPUT_GRADS) != 0;
    const bool dec_only = (flags & AVC_PLAN_DECODER_ONLY) != 0;
    const bool do_spk = has_spk(flags), do_enc = has_enc(flags), do_dec = has_dec(flags);
    if (int rc = check_model_cfg(*cfg, "avc_plan_create")) return rc;
    const avc_decoder_cfg& dc = cfg->dec;

    avc_plan* p = new avc_plan();
    p->cfg = *cfg;
    p->flags = flags;
    p->tun = tuning ? *tuning : avc_default_tuning();
    if (p->tun.wgrad_batch < 1) p->tun.wgrad_batch = 1;
    if (p->tun.wgrad_batch_wgs < 1) p->tun.wgrad_batch_wgs = 256;
    if (p->tun.wgrad_batch_units < 1) p->tun.wgrad_batch_units = 1L << 40;
    if (p->tun.dec_split_min < 2) p->tun.dec_split_min = 2;
    if (flags & AVC_PLAN_X3) {   // compute mode "fp32x3" 
        if (p->tun.conv_x3 < 1) p->tun.conv_x3 = 1;
        p->tun.wgrad_x3 = 1;
    }
    p->B = B;
    p->T = T;
    p->Tc = T_cond;
    p->M = cfg->enc.c_in;
    if (flags & AVC_PLAN_BF16S) {
        p->bh = true;
        p->compute = AVC_COMPUTE_BF16S;
        p->tun.conv_x3 = 0;
        p->tun.wgrad_x3 = 0;
        // schedule defaults of THIS mode (round 6, profiles/r06_bf16_schedule_sweep.log; the fp32 step measured both neutral or worse):
        // its weight gradients cost an eighth of the fp32 ones' matrix time, so (a) the decoder's go out UNDER the decoder's own latency-bound
        // backward chain, six layers at a time on 192 CUs, instead of being held behind the dense-stack kernel (2.44 - 2.46 vs 2.48 - 2.51 ms),
        // and (b) batches of 16 layers per stream-K launch (2.46 - 2.47 ms).  A caller's own values win: -1 = "held", any other batch size.
        if (p->tun.dec_wgrad_flush == 0) { p->tun.dec_wgrad_flush = 6; p->tun.dec_wgrad_wgs = 192; }
        if (p->tun.wgrad_batch == avc_default_tuning().wgrad_batch) p->tun.wgrad_batch = 16;
    }
    if (p->tun.dec_wgrad_flush < 0) p->tun.dec_wgrad_flush = 0;   // (-1: held, explicitly)

    // ---- parameters in reference registration order
    build_enc_params(p, p->spk, cfg->spk, true);
    p->enc_param_off = p->param_floats;
    build_enc_params(p, p->enc, cfg->enc, false);
    build_dec_params(p);
    DecNet& d = p->dec;

    // ---- time schedules + reflect-pad validity (reference raises the same way)
    auto sched_enc = [&](EncNet& e, int T0) -> int {
        e.T[0] = T0;
        int maxpad = e.c.bank_size / 2;
        if (maxpad >= T0) return -1;
        for (int l = 0; l < e.n; ++l) {
            if (e.c.kernel_size / 2 >= e.T[l]) return -1;
            e.T[l + 1] = avc_cdiv(e.T[l], e.c.subsample[l]);
        }
        return 0;
    };
    // (decoder part plans: T is the latent length Tb the caller hands in; the encoders' schedules do not exist)
    if (!dec_only && (sched_enc(p->spk, T_cond) || sched_enc(p->enc, T))) {
        delete p;
        return fail(-6, "Padding size should be less than the corresponding input dimension");
    }
    p->Tb = dec_only ? T : p->enc.T[p->enc.n];
    d.T[0] = p->Tb;
    for (int l = 0; l < d.n; ++l) {
        if (dc.kernel_size / 2 >= d.T[l]) {
            delete p;
            return fail(-6, "Padding size should be less than the corresponding input dimension");
        }
        d.T[l + 1] = d.T[l] * dc.upsample[l];
    }
    p->Tout = d.T[d.n];
    if (p->bh) {
        // pair rows: two channels per dword, four frames per 16-byte access of the row kernels
        bool ok = !((cfg->enc.c_in | cfg->enc.c_h | cfg->enc.c_bank | cfg->enc.c_out | cfg->spk.c_h | cfg->spk.c_bank | dc.c_h | dc.c_in | dc.c_out) & 1);
        if (!dec_only) {
            for (int l = 0; l <= p->spk.n; ++l) ok = ok && (p->spk.T[l] % 4 == 0);
            for (int l = 0; l <= p->enc.n; ++l) ok = ok && (p->enc.T[l] % 4 == 0);
            for (int l = 0; l < p->enc.n; ++l) ok = ok && (p->enc.T[l] <= 2048) && (p->spk.T[l] <= 2048);
        }
        for (int l = 0; l <= d.n; ++l) ok = ok && (d.T[l] % 4 == 0) && (d.T[l] <= 2048);
        if (!ok) {
            delete p;
            return fail(AVC_ERR_PAIR_SHAPE, "avc_plan_create: AVC_PLAN_BF16S needs even channel counts and frame counts that are multiples of 4 (<= 2048) at every level");
        }
    }

    // ---- packed weights (inference plans keep no dgrad images; part plans only their own network's)
    const bool dg = !infer;
    for (EncNet* e : {&p->spk, &p->enc}) {
        if (!(e == &p->enc ? do_enc : do_spk)) continue;
        for (int id : e->bank) finish_layer(p, p->layers[id], ig, 0, B, e->T[0], e->T[0], e->nb);
        finish_layer(p, p->layers[e->in_conv], dg, e->CC - e->c.c_in, B, e->T[0], e->T[0]);
        if (ig) {   // the in_conv's input gradient for its last M input rows (x itself, model.py:90): w[0] rows [nb c_bank, CC)
            LayerP L = p->layers[e->in_conv];
            L.src_off = (long)e->nb * e->c.c_bank;
            L.x3_f = L.x3_d = false;
            L.wpf = L.wrs_f = L.wrs_d = L.wplain = L.bpk = -1;
            L.need_dgrad = true;
            L.dgM = e->c.c_in;
            L.Mp_d = avc_cdiv(L.dgM, 128) * 128;
            const int td = avc_conv_pick_tile(p->tun, L.Mp_d, B, e->T[0], 1, L.Cout * L.KS);
            L.CKd = avc_conv_ck_for(p->tun, L.KS, avc_conv_num_wgs(td, L.Mp_d, B, e->T[0], 1), 1, L.stride, e->T[0], td);
            L.nchunk_d = avc_cdiv(L.bh ? L.Cout / 2 : L.Cout, L.CKd);
            L.wpd = p->alloc((long)L.nchunk_d * L.KS * L.CKd * L.Mp_d);
            p->layers.push_back(L);
            e->in_pass = (int)p->layers.size() - 1;
        }
        for (int l = 0; l < e->n; ++l) {
            finish_layer(p, p->layers[e->c1[l]], dg, 0, B, e->T[l], e->T[l]);
            finish_layer(p, p->layers[e->c2[l]], dg, 0, B, e->T[l + 1], e->T[l]);
        }
    }
    for (int l = 0; l < p->spk.nd && do_spk; ++l) {
        finish_layer(p, p->layers[p->spk.dn1[l]], dg, 0, 1, B, B, 1, false);
        finish_layer(p, p->layers[p->spk.dn2[l]], dg, 0, 1, B, B, 1, false);
    }
    if (do_spk) finish_layer(p, p->layers[p->spk.outl], dg, 0, 1, B, B, 1, false);
    if (do_enc) finish_layer(p, p->layers[p->enc.heads], dg, 0, B, p->Tb, p->Tb);
    if (do_dec) {
        finish_layer(p, p->layers[d.in_conv], dg, 0, B, p->Tb, p->Tb);
        for (int l = 0; l < d.n; ++l) {
            finish_layer(p, p->layers[d.c1[l]], dg, 0, B, d.T[l], d.T[l]);
            finish_layer(p, p->layers[d.c2[l]], dg, 0, B, d.T[l], d.T[l]);
        }
        finish_layer(p, p->layers[d.affine], dg, 0, 1, B, B, 1, true, false);
        if (dg) {   // d(emb) = W^T dcond runs through the weight-gradient kernel, which reads W as a plain [Kp][Mp] matrix
            LayerP& La = p->layers[d.affine];
            La.wplain = p->alloc((long)La.nchunk_f * La.CK * La.Mp_f);
        }
        finish_layer(p, p->layers[d.out_conv], dg, 0, B, p->Tout, p->Tout);
    }

    // ---- activations.  Inference plans (AVC_PLAN_INFERENCE) keep only what the forward pass touches;
    // part plans only their own network's buffers (in a whole plan's allocation order, minus the rest).
    const long Bl = B;
    const long H = p->bh ? 2 : 1;   // a stored [B, C, T] activation takes C / H dword rows per sample (bf16 pairs: half the floats)
    auto alloc_enc = [&](EncNet& e, bool spk) {
        const long C = e.c.c_h / H;
        e.cat = p->alloc(Bl * (e.CC / H) * e.T[0]);
        if (!infer) e.dcat = p->alloc(Bl * (e.CC / H) * e.T[0]);
        if (ig) e.dx = p->alloc(Bl * e.c.c_in * e.T[0]);
        e.h0 = p->alloc(Bl * C * e.T[0]);
        e.out[0] = spk ? e.h0 : p->alloc(Bl * C * e.T[0]);
        if (!spk) e.st0 = p->alloc(2 * Bl * e.c.c_h);
        for (int l = 0; l < e.n; ++l) {
            e.a1[l] = p->alloc(Bl * C * e.T[l]);
            e.out[l + 1] = p->alloc(Bl * C * e.T[l + 1]);
            if (spk) {
                e.a2[l] = p->alloc(Bl * C * e.T[l + 1]);
                e.y1[l] = e.y2[l] = -1;
            } else {
                e.a2[l] = -1;
                e.y1[l] = p->alloc(Bl * C * e.T[l]);
                e.y2[l] = p->alloc(Bl * C * e.T[l + 1]);
                e.st1[l] = p->alloc(2 * Bl * e.c.c_h);
                e.st2[l] = p->alloc(2 * Bl * e.c.c_h);
            }
        }
        if (spk) {   // (the dense stack is fp32)
            const long Cf = e.c.c_h;
            e.pooled = p->alloc(Cf * Bl);
            e.hd[0] = e.pooled;
            for (int l = 0; l < e.nd; ++l) {
                e.d1[l] = p->alloc(Cf * Bl);
                e.d2[l] = p->alloc(Cf * Bl);
                e.hd[l + 1] = p->alloc(Cf * Bl);
            }
        }
    };
    const long Cz = dc.c_in, Cd = dc.c_h;
    if (do_spk) {
        alloc_enc(p->spk, true);
        p->emb = p->alloc(Bl * dc.c_cond);
    }
    if (do_enc) {
        alloc_enc(p->enc, false);
        p->muls = p->alloc(Bl * 2 * Cz * p->Tb);
    }
    if (do_dec) {
        if (!dec_only || p->bh) d.z = p->alloc(Bl * (Cz / H) * p->Tb);   // (fp32 decoder part plans read the caller's z in place)
        d.cond = p->alloc(Bl * 2 * d.n * 2 * Cd);
        d.y0 = p->alloc(Bl * (Cd / H) * d.T[0]);
        d.out[0] = p->alloc(Bl * (Cd / H) * d.T[0]);
        d.st0 = p->alloc(2 * Bl * Cd);
        for (int l = 0; l < d.n; ++l) {
            d.y1[l] = p->alloc(Bl * (Cd / H) * d.T[l]);
            d.a1[l] = p->alloc(Bl * (Cd / H) * d.T[l]);
            d.y2[l] = p->alloc(Bl * (Cd / H) * d.T[l + 1]);
            d.out[l + 1] = p->alloc(Bl * (Cd / H) * d.T[l + 1]);
            d.st1[l] = p->alloc(2 * Bl * Cd);
            d.st2[l] = p->alloc(2 * Bl * Cd);
        }
        p->decb = p->alloc(Bl * p->M * p->Tout);
    }
    if (!infer) {
        if (do_enc) p->dmuls = p->alloc(Bl * 2 * Cz * p->Tb);
        if (do_spk || do_dec) p->demb = p->alloc(Bl * dc.c_cond);   // (speaker part plans: the caller's d(emb), channel-major)
        if (do_dec) {
            p->dz = p->alloc(Bl * Cz * p->Tb);
            d.dcond = p->alloc(Bl * 2 * d.n * 2 * Cd);
            p->ddec = p->alloc(Bl * p->M * p->Tout);
        }
        if (!part) {
            p->losses = p->alloc(64);
            p->loss_partial = p->alloc(2 * 1024);
        }
        // ---- gradient temporaries (sized for the largest [B, C, T] they ever hold)
        long maxCT = 0;
        auto upd = [&](long c, long t) { maxCT = ((c / H) * t > maxCT) ? (c / H) * t : maxCT; };
        for (int l = 0; l <= p->spk.n && do_spk; ++l) upd(p->spk.c.c_h, p->spk.T[l]);
        for (int l = 0; l <= p->enc.n && do_enc; ++l) upd(p->enc.c.c_h, p->enc.T[l]);
        for (int l = 0; l <= d.n && do_dec; ++l) upd(Cd, d.T[l]);
        if (do_dec) upd(p->M, p->Tout);
        if (do_enc || do_dec) {   // (the content branch's and the decoder's chains)
            p->gA = p->alloc(Bl * maxCT);
            p->gB = p->alloc(Bl * maxCT);
            p->gC = p->alloc(Bl * maxCT);
        }
        if (do_spk) {             // (the speaker branch's own set)
            p->gA2 = p->alloc(Bl * maxCT);
            p->gB2 = p->alloc(Bl * maxCT);
            p->gC2 = p->alloc(Bl * maxCT);
            p->dhA = p->alloc((long)p->spk.c.c_h * Bl);
        }
        if (p->bh) {
            if (do_dec) p->ddecp = p->alloc(Bl * p->M * p->Tout / 2);
            if (do_enc) p->dmulsp = p->alloc(Bl * Cz * p->Tb);
        }
        if (dec_only) p->demb_rm = p->alloc(Bl * dc.c_cond);
    }

    if (do_spk) {
        p->named["emb"] = p->emb;
        p->named["spk_cat"] = p->spk.cat;
        p->named["spk_out0"] = p->spk.out[0];
        p->named["spk_pooled"] = p->spk.pooled;
        p->named["spk_outN"] = p->spk.out[p->spk.n];
    }
    if (do_enc) {
        p->named["muls"] = p->muls;
        p->named["enc_cat"] = p->enc.cat;
        p->named["enc_out0"] = p->enc.out[0];
        p->named["enc_outN"] = p->enc.out[p->enc.n];
    }
    if (do_dec) {
        p->named["dec"] = p->decb;
        if (d.z >= 0) p->named["z"] = d.z;
        p->named["cond"] = d.cond;
        p->named["dec_out0"] = d.out[0];
        p->named["dec_outN"] = d.out[d.n];
    }
    if (!infer) {
        if (!part) p->named["losses"] = p->losses;
        if (do_enc) p->named["d_muls"] = p->dmuls;
        if (do_dec) {
            p->named["d_dec"] = p->ddec;
            p->named["d_z"] = p->dz;
            p->named["d_emb"] = dec_only ? p->demb_rm : p->demb;
            p->named["d_cond"] = d.dcond;
        }
        if (ig) {
            p->named["d_x"] = do_enc ? p->enc.dx : p->spk.dx;
            if (do_enc && do_spk) p->named["d_x_cond"] = p->spk.dx;
        }
    }

    // ---- ReLU site table in the reference's forward call order (avc_plan_relu_site).  Pair plans: activation / conv-output tensors
    // are bf16 pair tensors (storage 1: strides in dwords) or, after a pixel-shuffling conv, natural bf16 rows (storage 2)
    {
        const long H = p->bh ? 2 : 1;   // channels per row of a stored [B, C, T] tensor
        auto conv_site = [&](long off, int Bn, int C, int T, long sb, long sc, long st, int storage) {
            avc_relu_site r;
            memset(&r, 0, sizeof(r));
            r.kind = 0; r.B = Bn; r.C = C; r.T = T; r.act_off = off; r.sb = sb; r.sc = sc; r.st = st;
            r.y_off = r.stat_off = r.cond_off = -1;
            r.storage = storage;
            p->sites.push_back(r);
        };
        auto in_site = [&](long y, long st, int C, int T, long cond, long csb, int storage) {
            avc_relu_site r;
            memset(&r, 0, sizeof(r));
            r.kind = 1; r.B = B; r.C = C; r.T = T; r.act_off = -1;
            r.y_off = y; r.stat_off = st; r.cond_off = cond; r.cond_sb = csb;
            r.storage = storage;
            p->sites.push_back(r);
        };
        const int PS = p->bh ? 1 : 0;
        const EncNet& sp = p->spk;
        const int Cs_ = sp.c.c_h;
        if (do_spk) {
            for (int g = 0; g < sp.nb; ++g) conv_site(sp.cat + (long)g * (sp.c.c_bank / H) * sp.T[0], B, sp.c.c_bank, sp.T[0], (long)(sp.CC / H) * sp.T[0], sp.T[0], 1, PS);
            conv_site(sp.h0, B, Cs_, sp.T[0], (long)(Cs_ / H) * sp.T[0], sp.T[0], 1, PS);
            for (int l = 0; l < sp.n; ++l) {
                conv_site(sp.a1[l], B, Cs_, sp.T[l], (long)(Cs_ / H) * sp.T[l], sp.T[l], 1, PS);
                conv_site(sp.a2[l], B, Cs_, sp.T[l + 1], (long)(Cs_ / H) * sp.T[l + 1], sp.T[l + 1], 1, PS);
            }
            for (int l = 0; l < sp.nd; ++l) {  // dense activations are stored channel-major [C][B] fp32; the reference sees [B, C]
                conv_site(sp.d1[l], B, Cs_, 1, 1, B, 0, 0);
                conv_site(sp.d2[l], B, Cs_, 1, 1, B, 0, 0);
            }
        }
        const EncNet& en = p->enc;
        const int Ce_ = en.c.c_h;
        if (do_enc) {
            for (int g = 0; g < en.nb; ++g) conv_site(en.cat + (long)g * (en.c.c_bank / H) * en.T[0], B, en.c.c_bank, en.T[0], (long)(en.CC / H) * en.T[0], en.T[0], 1, PS);
            in_site(en.h0, en.st0, Ce_, en.T[0], -1, 0, PS);
            for (int l = 0; l < en.n; ++l) {
                in_site(en.y1[l], en.st1[l], Ce_, en.T[l], -1, 0, PS);
                in_site(en.y2[l], en.st2[l], Ce_, en.T[l + 1], -1, 0, PS);
            }
        }
        if (do_dec) {
            const long csb_ = (long)2 * d.n * 2 * Cd;
            in_site(d.y0, d.st0, (int)Cd, d.T[0], -1, 0, PS);
            for (int l = 0; l < d.n; ++l) {
                in_site(d.y1[l], d.st1[l], (int)Cd, d.T[l], d.cond + (long)(2 * l) * 2 * Cd, csb_, PS);
                in_site(d.y2[l], d.st2[l], (int)Cd, d.T[l + 1], d.cond + (long)(2 * l + 1) * 2 * Cd, csb_, (p->bh && dc.upsample[l] > 1) ? 2 : PS);
            }
        }
    }

    // ---- split-K slabs, dy arena and the event pool: sized with a dry run of the backward pass
    if (!infer) {
        p->slab = p->ws_top;
        long need[3] = {0, 0, 0};
        avc_backward_impl(p, nullptr, nullptr, 0, 0, 0, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, 0.f, nullptr,
                          nullptr, nullptr, true, need);
        p->slab_floats = need[0];
        p->ws_top += (need[0] + 63) / 64 * 64;
        p->dyarena = p->ws_top;
        p->dyarena_floats = need[1];
        p->ws_top += (need[1] + 63) / 64 * 64;
        p->nev_need = (int)need[2];
        p->named["wgrad_slab"] = p->slab;      // (diagnostic views: scripts/bf16_repro_probe3.py)
        p->named["dy_arena"] = p->dyarena;
        p->named["g_tmp"] = p->gA;
    }
    // helper streams / events belong to the plan from here on (created on the device that is current NOW;
    // a process without a GPU -- host-only plan queries -- simply gets a single-stream plan)
    plan_init_streams(p);
    *out = p;
    return 0;
}

extern "C" void avc_plan_destroy(avc_plan* p) {
    if (!p) return;
    if (p->pack_tab_dev) hipFree(p->pack_tab_dev);
    if (p->pack_blk_dev) hipFree(p->pack_blk_dev);
    // every handle that exists, whatever state plan_init_streams ended in
    // (the helper streams belong to the device's shared set: shared_streams())
    if (p->ev_fork) hipEventDestroy(p->ev_fork);
    if (p->ev_join) hipEventDestroy(p->ev_join);
    for (int i = 0; i < 2; ++i) {
        if (p->wjoin[i]) hipEventDestroy(p->wjoin[i]);
    }
    for (hipEvent_t e : p->wev)
        if (e) hipEventDestroy(e);
    if (p->ev_dense) hipEventDestroy(p->ev_dense);
    if (p->ev_dec_grads) hipEventDestroy(p->ev_dec_grads);
    if (p->ev_spk_grads) hipEventDestroy(p->ev_spk_grads);
    if (p->ev_all_grads) hipEventDestroy(p->ev_all_grads);
    delete p;
}

// fork/join helpers: `side` runs one independent branch while the caller's stream runs the other
extern "C" int avc_plan_set_single_stream(avc_plan* p, int on) {
    if (!p) return fail(-1, "avc_plan_set_single_stream: null plan");
    p->tun.single_stream = on ? 1 : 0;
    return 0;
}

extern "C" int avc_plan_set_compute_dtype(avc_plan* p, int dtype) {
    if (!p || (dtype != AVC_COMPUTE_F32 && dtype != AVC_COMPUTE_BF16)) return fail(-1, "avc_plan_set_compute_dtype: dtype must be 0 (fp32) or 1 (bf16 operands)");
    if (p->bh) return fail(-1, "avc_plan_set_compute_dtype: the plan was created with AVC_PLAN_BF16S (bf16 storage is a property of the workspace layout)");
    p->compute = dtype;
    for (LayerP& L : p->layers) L.bf16 = dtype;
    return 0;
}
extern "C" int avc_plan_compute_dtype(const avc_plan* p) { return p ? p->compute : -1; }

static void pack_layer(const avc_plan* p, const LayerP& L, const float* params, float* ws, std::vector<PackArgs>& out);
static void plan_init_pack_table(avc_plan* p) {
    // descriptors against NULL bases: every pointer field then holds a byte offset
    // The conv banks and in_convs open both encoder branches and run for ~1 ms: their images come first (a short launch on the caller's
    // stream); everything else can be packed on a forward-idle helper stream UNDER those convolutions.
    std::vector<char> early(p->layers.size(), 0);
    if (!(p->flags & AVC_PLAN_RAGGED))
        for (const EncNet* e : {&p->spk, &p->enc}) {
            if (e->in_conv < 0) continue;
            for (int g = 0; g < e->nb; ++g) early[e->bank[g]] = 1;
            early[e->in_conv] = 1;
        }
    std::vector<PackArgs> all;
    for (int pass = 0; pass < 2; ++pass) {
        for (size_t i = 0; i < p->layers.size(); ++i)
            if ((p->layers[i].wpf >= 0 || p->layers[i].wpd >= 0) && (early[i] != 0) == (pass == 0)) pack_layer(p, p->layers[i], (const float*)nullptr, (float*)nullptr, all);
        if (pass == 0) p->pack_early_imgs = (int)all.size();
    }
    if (all.empty()) return;
    double bytes = 0;
    std::vector<int> blk;   // (image, piece) pairs
    for (size_t i = 0; i < all.size(); ++i) {
        if ((int)i == p->pack_early_imgs) p->pack_nblk_early = (int)(blk.size() / 2);
        all[i].mb = avc_pack_stage_rows(all[i]);
        bytes += 8.0 * avc_pack_total(all[i]);
        const long np = avc_pack_pieces(all[i]);
        for (long q = 0; q < np; ++q) {
            blk.push_back((int)i);
            blk.push_back((int)q);
        }
    }
    if (p->pack_early_imgs >= (int)all.size()) p->pack_nblk_early = (int)(blk.size() / 2);
    PackArgs* dev = nullptr;
    void* dblk = nullptr;
    if (hipMalloc((void**)&dev, all.size() * sizeof(PackArgs)) != hipSuccess || hipMalloc(&dblk, blk.size() * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();   // no device (host-only plan queries): forward packs with descriptor batches in kernel arguments instead
        if (dev) hipFree(dev);
        return;
    }
    if (hipMemcpy(dev, all.data(), all.size() * sizeof(PackArgs), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dblk, blk.data(), blk.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        hipFree(dev);
        hipFree(dblk);
        return;
    }
    p->pack_tab_dev = dev;
    p->pack_blk_dev = dblk;
    p->pack_nblk = (int)(blk.size() / 2);
    p->pack_tab_bytes = bytes;
}

// The three helper streams of a plan -- the side branch's and the two weight-gradient streams -- are ONE set per device, shared by every plan
// of the process and kept for its lifetime (round 5).  The runtime deals streams to a handful of hardware queues in creation order: the
// first plan's three streams and the caller's stream take four of them, a second plan's OWN three land wherever the round-robin has got
// to -- its side stream on the caller's queue, for one: both branches of a pass then run one after the other (bf16 step 4.9 - 6.1 instead of
// 2.59 ms, measured: scripts/two_plans_probe.py).  All three are created together, in a fixed order, by the FIRST plan of the device; the side
// stream's priority is that plan's `side_prio` and stays: a later plan that asks for the other priority gets the existing stream (round 6: a
// fourth helper stream created later put the process back into the queue lottery -- 8.2 instead of 5.9 ms per step,
// profiles/r05_two_plans_probe.log -- so there is none; avc_plan_side_priority reports what a plan really runs with).
// Consequences for callers (include/avc_hip.h says the same): the helper streams are process-lifetime objects; two plans driven from two
// host threads share them, i.e. their side-branch / weight-gradient work is serialised stream by stream (every wait is on an event recorded
// earlier: ordering, never a hazard).  Immutable once created; the lookup is mutex-protected.
#ifndef AVC_EMU
#include <mutex>
#endif
struct DevStreams {
    hipStream_t side = nullptr;
    hipStream_t w[2] = {nullptr, nullptr};
    int side_prio = -1;   // priority class the side stream was created with (0 normal, 1 highest); -1: not created
};
static bool shared_streams(int side_prio, hipStream_t* side, hipStream_t* w0, hipStream_t* w1, int* prio_used) {
#ifdef AVC_EMU
    static DevStreams pool[1];
    const int dev = 0;
#else
    static std::mutex mu;
    static DevStreams pool[64];
    std::lock_guard<std::mutex> lk(mu);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
        (void)hipGetLastError();
        return false;
    }
#endif
    DevStreams& d = pool[dev];
    if (d.side_prio < 0) {
        int lo = 0, hi = 0;
        hipDeviceGetStreamPriorityRange(&lo, &hi);  // lo = least urgent, hi = most urgent
        const int sp = side_prio ? 1 : 0;
        // the side stream carries the speaker-encoder branch: the LONGER pole of both passes (forward: pooling + the latency-bound dense stack
        // after its convs, before the decoder can start; backward: d_emb -> dense stack -> its whole dgrad chain -> the last weight gradients).
        // side_prio = 1 dispatches its workgroups ahead of the content branch's and the weight-gradient streams'.
        hipStream_t s_ = nullptr, w_[2] = {nullptr, nullptr};
        bool ok = (sp ? hipStreamCreateWithPriority(&s_, hipStreamNonBlocking, hi) : hipStreamCreateWithFlags(&s_, hipStreamNonBlocking)) == hipSuccess;
        for (int i = 0; i < 2 && ok; ++i) ok = hipStreamCreateWithPriority(&w_[i], hipStreamNonBlocking, lo) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();  // no device: single-stream plan
            if (s_) hipStreamDestroy(s_);
            for (int i = 0; i < 2; ++i)
                if (w_[i]) hipStreamDestroy(w_[i]);
            return false;
        }
        d.side = s_; d.w[0] = w_[0]; d.w[1] = w_[1];
        d.side_prio = sp;
    }
    *side = d.side; *w0 = d.w[0]; *w1 = d.w[1];
    *prio_used = d.side_prio;
    return true;
}

static void plan_init_streams(avc_plan* p) {
    plan_init_pack_table(p);
    p->side_state = -1;
    int prio_used = p->tun.side_prio ? 1 : 0;
    if (!shared_streams(p->tun.side_prio, &p->side, &p->wstream[0], &p->wstream[1], &prio_used)) {
        p->side = nullptr;
        p->wstream[0] = p->wstream[1] = nullptr;
        return;
    }
    bool ok = hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&p->ev_join, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&p->ev_dense, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&p->ev_dec_grads, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&p->ev_spk_grads, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&p->ev_all_grads, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 2; ++i) {
        ok = ok && hipEventCreateWithFlags(&p->wjoin[i], hipEventDisableTiming) == hipSuccess;
    }
    p->wev.assign((size_t)p->nev_need, nullptr);
    for (hipEvent_t& e : p->wev) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    p->side_state = ok ? 1 : -1;
    p->tun.side_prio = prio_used;   // (what the device's shared side stream really has)
}
static bool side_ready(const avc_plan* p) { return !p->tun.single_stream && p->side_state == 1; }
static hipStream_t fork_side(const avc_plan* p, hipStream_t mainS) {
    if (!side_ready(p)) return mainS;
    hipEventRecord(p->ev_fork, mainS);
    hipStreamWaitEvent(p->side, p->ev_fork, 0);
    return p->side;
}
static void join_side(const avc_plan* p, hipStream_t mainS, hipStream_t sideS) {
    if (sideS == mainS) return;
    hipEventRecord(p->ev_join, sideS);
    hipStreamWaitEvent(mainS, p->ev_join, 0);
}
extern "C" int avc_plan_side_priority(const avc_plan* p) { return p->side_state == 1 ? p->tun.side_prio : -1; }
extern "C" int avc_plan_num_params(const avc_plan* p) { return (int)p->params.size(); }
extern "C" long avc_plan_param_floats(const avc_plan* p) { return p->param_floats; }
extern "C" int avc_plan_param_info(const avc_plan* p, int i, long* offset, long* numel, int dims[3]) {
    if (i < 0 || i >= (int)p->params.size()) return -1;
    *offset = p->params[i].off;
    *numel = p->params[i].numel;
    for (int k = 0; k < 3; ++k) dims[k] = p->params[i].d[k];
    return 0;
}
extern "C" long avc_plan_workspace_floats(const avc_plan* p) { return p->ws_top; }
extern "C" long avc_plan_buffer(const avc_plan* p, const char* name) {
    auto it = p->named.find(name);
    return it == p->named.end() ? -1 : it->second;
}
extern "C" int avc_plan_num_relu_sites(const avc_plan* p) { return (int)p->sites.size(); }
extern "C" int avc_plan_relu_site(const avc_plan* p, int i, avc_relu_site* out) {
    if (i < 0 || i >= (int)p->sites.size()) return -1;
    *out = p->sites[i];
    return 0;
}
extern "C" int avc_plan_flags(const avc_plan* p) { return p ? p->flags : -1; }
// Data-parallel hook: the decoder's parameters are the tail of the flat buffer and their
// gradients are final well before the encoders' (the backward pass walks decoder -> encoders).
extern "C" int avc_plan_param_range(const avc_plan* p, int part, long* offset, long* numel) {
    if (!p || !offset || !numel) return -1;
    if (part == AVC_GRADS_DECODER) {
        *offset = p->dec_param_off;
        *numel = p->param_floats - p->dec_param_off;
    } else if (part == AVC_GRADS_ENCODERS) {
        *offset = 0;
        *numel = p->dec_param_off;
    } else if (part == AVC_GRADS_SPEAKER) {
        *offset = 0;
        *numel = p->enc_param_off;
    } else if (part == AVC_GRADS_CONTENT) {
        *offset = p->enc_param_off;
        *numel = p->dec_param_off - p->enc_param_off;
    } else if (part == AVC_GRADS_ALL) {
        *offset = 0;
        *numel = p->param_floats;
    } else {
        return -1;
    }
    return 0;
}
// make `stream` wait until the gradients of `part` written by the LAST avc_backward call on this plan are final
// (a no-op before the first call).  -9: the plan could not create helper streams / events -- nothing was ordered, the
// caller must make `stream` wait for the stream avc_backward ran on.
extern "C" int avc_plan_stream_wait_grads(const avc_plan* p, int part, void* stream) {
    if (!p || (p->flags & AVC_PLAN_INFERENCE)) return fail(-1, "avc_plan_stream_wait_grads: not a training plan");
    if (p->side_state != 1) return fail(-9, "avc_plan_stream_wait_grads: the plan has no helper streams / events (order on the stream avc_backward ran on)");
    hipEvent_t e = (part == AVC_GRADS_DECODER) ? p->ev_dec_grads : (part == AVC_GRADS_SPEAKER ? p->ev_spk_grads : p->ev_all_grads);
    return (int)hipStreamWaitEvent((hipStream_t)stream, e, 0);
}
extern "C" int avc_plan_out_len(const avc_plan* p) { return p->Tout; }
extern "C" int avc_plan_latent_len(const avc_plan* p) { return p->Tb; }

// --------------------------------------------------------------------------
// launch helpers
// --------------------------------------------------------------------------
static void set_group(ConvGroup& g, const float* wp, const float* bias, int KS, int CK, int nchunk) {
    memset(&g, 0, sizeof(g));
    g.wp = wp;
    g.bias = bias;
    g.KS = KS;
    g.padL = KS / 2;
    g.padR = (KS % 2 == 0) ? KS / 2 - 1 : KS / 2;
    g.CK = CK;
    g.nchunk = nchunk;
}

static const float* layer_bias(const avc_plan* p, const LayerP& L, const float* params, const float* ws) {
    return L.nsrc == 1 ? p->par(params, L.b[0]) : ws + L.bpk;
}

// forward conv of layer L on a source view; caller fills epilogue extras afterwards
static ConvArgs mk_fwd(const avc_plan* p, float slope, const LayerP& L, const float* params, const float* ws, const float* x, long sb,
                       long sc, int st, int Bn, int Tsrc, float* out, long ob, long oc, int ot, int act) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.x.ptr = x; a.x.sb = sb; a.x.sc = sc; a.x.st = st; a.x.ps = 1;
    a.B = Bn; a.Cred = L.bh ? L.Cin / 2 : L.Cin; a.Tsrc = Tsrc;
    a.mode = 0; a.stride = L.stride; a.bf16 = L.bf16;
    a.pairs = L.bh ? 1 : 0;   // (callers clear it for the fp32 outputs of the heads and the decoder's last conv)
    a.M = L.Cout; a.Mp = L.Mp_f;
    a.ngroups = 1;
    set_group(a.g[0], ws + (L.x3_f ? L.wrs_f : L.wpf), layer_bias(p, L, params, ws), L.KS, L.CK, L.nchunk_f);
    a.img = L.x3_f ? AVC_IMG_X3 : (L.bh ? AVC_IMG_K4H : AVC_IMG_K4);
    a.Tout = (Tsrc + a.g[0].padL + a.g[0].padR - L.KS) / L.stride + 1;
    a.ob = ob; a.oc = oc; a.ot = ot; a.ops = 1;
    a.act = act;
    a.slope = slope;
    a.g[0].out = out;
    return a;
}

static ConvArgs mk_dgrad(float slope, const LayerP& L, const float* ws, const float* dy, long sb, long sc, int st, int ps, int Bn,
                         int Tdy, int Tin, float* dx, long ob, long oc, int ot) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.x.ptr = dy; a.x.sb = sb; a.x.sc = sc; a.x.st = st; a.x.ps = ps;
    a.B = Bn; a.Cred = L.bh ? L.Cout / 2 : L.Cout; a.Tsrc = Tdy;
    a.pairs = L.bh ? 1 : 0;
    a.mode = 1; a.stride = L.stride; a.mirror = (L.KS > 1) ? 1 : 0; a.bf16 = L.bf16;
    a.M = L.dgM; a.Mp = L.Mp_d; a.Tout = Tin;
    a.ob = ob; a.oc = oc; a.ot = ot; a.ops = 1;
    a.res_to_primary = 1;
    a.slope = slope;   // (applied where the launch masks by a ReLU output)
    a.ngroups = 1;
    set_group(a.g[0], ws + (L.x3_d ? L.wrs_d : L.wpd), nullptr, L.KS, L.CKd, L.nchunk_d);
    a.img = L.x3_d ? AVC_IMG_X3 : (L.bh ? AVC_IMG_K4H : AVC_IMG_K4);
    a.g[0].out = dx;
    return a;
}

static void set_res(ConvArgs& a, const float* res, int mode, long rb, long rc, int rt, int Tres) {
    a.g[0].res = res;
    a.res_mode = mode;
    a.rb = rb; a.rc = rc; a.rt = rt; a.Tres = Tres;
}

// The speaker encoder's dense stack (dense blocks + output layer) as the ONE fused launch of dense.hip reads it: the forward images and
// biases, or (backward; params may be NULL) the input-gradient images.  No side effects.  Callers add the ends of their pass: in, emb and
// the blocks' out2 (forward); in, dpooled and the layers' dz (backward).
static DenseArgs dense_stack_args(const avc_plan* p, const EncNet& e, const float* params, float* ws, bool backward) {
    DenseArgs a;
    memset(&a, 0, sizeof(a));
    a.nlayers = 2 * e.nd + 1;
    a.B = p->B; a.C = e.c.c_h; a.slope = e.slope;
    for (int l = 0; l < a.nlayers; ++l) {
        const bool last = (l == a.nlayers - 1);
        const LayerP& L = p->layers[last ? e.outl : ((l & 1) ? e.dn2[l / 2] : e.dn1[l / 2])];
        DenseLayer& D = a.layer[l];
        D.wp = ws + (backward ? L.wpd : L.wpf);
        if (!backward) D.bias = p->par(params, L.b[0]);
        D.Cin = L.Cin; D.Cout = L.Cout; D.Mp = backward ? L.Mp_d : L.Mp_f;
        D.Kp = backward ? L.nchunk_d * L.CKd : L.nchunk_f * L.CK;
        if (!last) D.act = ws + ((l & 1) ? e.d2[l / 2] : e.d1[l / 2]);
        a.Kmax = D.Kp > a.Kmax ? D.Kp : a.Kmax;
        a.Wmax = D.Kp * D.Mp > a.Wmax ? D.Kp * D.Mp : a.Wmax;
    }
    return a;
}

struct BwdCtx {
    const avc_plan* p;
    const float* params;
    float* grads;
    float* ws;
    hipStream_t s;
    bool dry;
    long slab_used;
    hipStream_t wstream;   // stream of the weight-gradient kernels of the current branch (== s when not overlapping)
    int nev;
    long dy_used;
    // weight gradients recorded but not launched yet: they run as batched launches (conv_wgrad.hip) once
    // p->wgrad_batch layers are pending or a branch ends -- few large, balanced launches with short split-K
    // instead of one launch per layer
    struct PendW {
        WgradArgs a;
        const LayerP* L;
    };
    std::vector<PendW> pend;
    bool hold = false;     // keep recording (no automatic flush): the decoder's layers go out together, behind the dense-stack kernel
    hipStream_t s_extra = nullptr;   // a second producer stream the next flush must also be ordered behind (the decoder's other half-batch chain)
    int target_wgs = 0;              // workgroups per launch of the next flush (0 = avc_tuning.wgrad_batch_wgs)
    long pend_units = 0;   // (co, ci) tiles x K-chunks of the pending layers
    // every gradient tensor a (possibly still running) wgrad kernel reads gets its own buffer
    float* fresh(long n) {
        long off = dy_used;
        dy_used += (n + 63) / 64 * 64;
        return dry ? nullptr : ws + p->dyarena + off;
    }
};

// One ordering edge "everything queued on c.s so far -> the branch's wgrad stream"; returns the stream
// to launch on.  Edges are counted in the dry run too: that count sizes the plan's event pool, so the
// index is always valid at run time.
static hipStream_t wgrad_edge(BwdCtx& c, bool two_producers = false) {
    const int i = c.nev++;
    const int i2 = two_producers ? c.nev++ : -1;   // (counted in the dry run whether or not the second stream exists at run time)
    if (c.dry || c.wstream == c.s) return c.s;
    hipEvent_t e = c.p->wev[i];
    hipEventRecord(e, c.s);
    hipStreamWaitEvent(c.wstream, e, 0);
    if (two_producers && c.s_extra && c.s_extra != c.s) {
        hipEvent_t e2 = c.p->wev[i2];
        hipEventRecord(e2, c.s_extra);
        hipStreamWaitEvent(c.wstream, e2, 0);
    }
    return c.wstream;
}

// Launch the pending weight gradients of this branch on the branch's wgrad stream (ordered behind everything queued on c.s so far:
// their dy operands are final): one stream-K launch per kernel instance present (conv_wgrad.hip) + ONE reduce launch that sums the
// partial tiles in a fixed order into the flat gradient buffer (weights and biases).  Runs beside the dgrad / InstanceNorm-backward chain.
static int flush_wgrads(BwdCtx& c, bool two_producers = false) {
    if (c.pend.empty()) return 0;
    hipStream_t ls = wgrad_edge(c, two_producers);
    const int n = (int)c.pend.size();
    std::vector<WgradArgs> L((size_t)n);
    for (int i = 0; i < n; ++i) L[i] = c.pend[i].a;
    avc_wgrad_plan_batch(L.data(), n, c.target_wgs > 0 ? c.target_wgs : c.p->tun.wgrad_batch_wgs);
    for (int i = 0; i < n; ++i) {
        WgradArgs& a = L[i];
        const long off = c.slab_used;
        c.slab_used += (a.slab_need + a.dbslab_need + 63) / 64 * 64;
        if (c.dry) continue;
        a.slab = c.ws + c.p->slab + off;
        a.dbslab = a.slab + a.slab_need;
        const LayerP& Lp = *c.pend[i].L;
        a.rows_per_src = Lp.rows;
        a.dw = c.grads + c.p->params[Lp.w[0]].off;
        a.db = c.grads + c.p->params[Lp.b[0]].off;
        a.dw_src_stride = Lp.nsrc > 1 ? c.p->params[Lp.w[1]].off - c.p->params[Lp.w[0]].off : 0;
        a.db_src_stride = Lp.nsrc > 1 ? c.p->params[Lp.b[1]].off - c.p->params[Lp.b[0]].off : 0;
    }
    c.pend.clear();
    c.pend_units = 0;
    if (c.dry) return 0;
    return avc_launch_wgrad_batch(L.data(), n, ls, c.p->tun.wgrad_ablation);
}

// weight + bias gradient of layer L: x = forward input view, dy = output-gradient view (recorded; see flush_wgrads)
static int wgrad_layer(BwdCtx& c, const LayerP& L, const float* x, long xsb, long xsc, int xst, const float* dy, long ysb,
                       long ysc, int yst, int yps, int Bn, int Tin, int Tout) {
    BwdCtx::PendW pw;
    WgradArgs& a = pw.a;
    memset(&a, 0, sizeof(a));
    a.x.ptr = x; a.x.sb = xsb; a.x.sc = xsc; a.x.st = xst; a.x.ps = 1;
    a.dy.ptr = dy; a.dy.sb = ysb; a.dy.sc = ysc; a.dy.st = yst; a.dy.ps = yps;
    a.B = Bn; a.Cin = L.Cin; a.Cout = L.Cout; a.Tin = Tin; a.Tout = Tout;
    a.KS = L.KS; a.padL = L.KS / 2; a.stride = L.stride;
    a.bf16 = (L.bf16 == AVC_COMPUTE_F32 && c.p->tun.wgrad_x3) ? AVC_COMPUTE_F32X3 : L.bf16;
    a.cw8 = c.p->tun.wgrad_cw8 ? 1 : 0;
    pw.L = &L;
    avc_wgrad_geometry(a);
    c.pend_units += (long)a.tiles * a.total_chunks;
    c.pend.push_back(pw);
    // flush when the batch is worth a launch: enough work to give every CU a long K run, or enough layers
    if (!c.hold && ((int)c.pend.size() >= c.p->tun.wgrad_batch || c.pend_units >= c.p->tun.wgrad_batch_units)) return flush_wgrads(c);
    return 0;
}

static void pack_layer(const avc_plan* p, const LayerP& L, const float* params, float* ws, std::vector<PackArgs>& out) {
    PackArgs a;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < L.nsrc; ++i) a.src[i] = p->par(params, L.w[i]);
    a.src[0] += L.src_off;   // (rows [src_off, src_off + dgM) of a forward input: the pack's input-gradient index stays below Cout Cin KS)
    a.nsrc = L.nsrc; a.rows_per_src = L.rows;
    a.Cout = L.Cout; a.Cin = L.Cin; a.KS = L.KS;
    a.dgrad = 0; a.CK = L.CK; a.nchunk = L.nchunk_f; a.M = L.Cout; a.Mp = L.Mp_f;
    a.dst = ws + L.wpf;
    a.img = L.conv_path ? (L.bh ? AVC_IMG_K4H : AVC_IMG_K4) : AVC_IMG_PLAIN;
    if (L.wpf < 0) {
        // (an input-gradient image only: EncNet::in_pass)
    } else if (L.x3_f) {   // only the image the launch will read
        PackArgs r;
        avc_pack_x3_args(r, p->par(params, L.w[0]), L.Cout, L.Cin, L.KS, 0, ws + L.wrs_f);
        out.push_back(r);
    } else {
        out.push_back(a);
    }
    if (L.wplain >= 0) {
        PackArgs b = a;
        b.img = AVC_IMG_PLAIN;
        b.dst = ws + L.wplain;
        out.push_back(b);
    }
    if (L.need_dgrad && L.x3_d) {
        PackArgs r;
        avc_pack_x3_args(r, p->par(params, L.w[0]), L.Cout, L.Cin, L.KS, 1, ws + L.wrs_d, L.dgM);
        out.push_back(r);
    } else if (L.need_dgrad) {
        a.dgrad = 1; a.CK = L.CKd; a.nchunk = L.nchunk_d; a.M = L.dgM; a.Mp = L.Mp_d;
        a.dst = ws + L.wpd;
        out.push_back(a);
    }
    if (L.nsrc > 1) {  // stacked bias = "weight" with Cin = 1, KS = 1: first Mp floats of the plain image
        PackArgs b;
        memset(&b, 0, sizeof(b));
        for (int i = 0; i < L.nsrc; ++i) b.src[i] = p->par(params, L.b[i]);
        b.nsrc = L.nsrc; b.rows_per_src = L.rows;
        b.Cout = L.Cout; b.Cin = 1; b.KS = 1;
        b.dgrad = 0; b.CK = 32; b.nchunk = 1; b.M = L.Cout; b.Mp = L.Mp_f;
        b.dst = ws + L.bpk;
        b.img = AVC_IMG_PLAIN;
        out.push_back(b);
    }
}

static int in_fwd(float slope, const float* y, int Bn, int C, int T, const float* cond, long cond_sb, int cond_off, const float* res,
                  int res_mode, int Tres, float* out, float* stats, hipStream_t s, int Bfull = 0, int b0 = 0, bool pairs = false, int planar = 0, int nv = 0) {
    // stats = [mean[Bfull*C] | rstd[Bfull*C]]; a sub-batch launch (b0, Bn) of a Bfull-sample tensor passes
    // y/out/res/cond already offset to sample b0
    if (Bfull == 0) Bfull = Bn;
    INFwdArgs a;
    a.y = y; a.out = out; a.mean = stats + (long)b0 * C; a.rstd = stats + (long)Bfull * C + (long)b0 * C;
    a.cond = cond; a.cond_sb = cond_sb; a.cond_off = cond_off;
    a.res = res; a.res_mode = res ? res_mode : 0; a.Tres = Tres;
    a.R = Bn * C; a.C = C; a.T = T; a.relu = 1; a.slope = slope; a.planar = planar; a.nv_hint = nv;
    if (pairs) {
        a.R = Bn * (C / 2);
        return avc_launch_in_fwd_pairs(a, s);
    }
    return avc_launch_in_fwd(a, s);
}

// conv + the InstanceNorm rows of its output: inside the conv's epilogue where a 64-column tile holds whole rows (avc_conv_in_fusable:
// rows of 16 / 32 / 64 frames, exact fp32), else the row kernel behind the conv.  a.g[0].out = y (pre-norm, read by the backward pass).
static int conv_in_fwd(const avc_plan* p, ConvArgs& a, float slope, int Bn, int C, int T, const float* cond, long cond_sb, int cond_off,
                       const float* res, int res_mode, int Tres, float* out, float* stats, hipStream_t s, int Bfull = 0, int b0 = 0,
                       bool pairs = false, int planar = 0, int nv = 0) {
    if (Bfull == 0) Bfull = Bn;
    if (!planar && avc_conv_in_fusable(a, p->tun, res ? res_mode : AVC_RES_NONE, Tres)) {   // (pair tensors too; a pixel-shuffling conv's "planar" rows keep the row kernel)
        a.in.out = out;
        a.in.mean = stats + (long)b0 * C;
        a.in.rstd = stats + (long)Bfull * C + (long)b0 * C;
        a.in.cond = cond; a.in.cond_sb = cond_sb; a.in.cond_off = cond_off;
        a.in.res = res; a.in.res_mode = res ? res_mode : 0; a.in.Tres = Tres;
        a.in.C = C; a.in.relu = 1;
        return avc_launch_conv(a, s, 0, p->tun);
    }
    int rc = avc_launch_conv(a, s, 0, p->tun);
    if (rc) return rc;
    return in_fwd(slope, a.g[0].out, Bn, C, T, cond, cond_sb, cond_off, res, res_mode, Tres, out, stats, s, Bfull, b0, pairs, planar, nv);
}

static int in_bwd(float slope, const float* g, const float* y, const float* stats, int Bn, int C, int T, const float* cond,
                  long cond_sb, int cond_off, float* dy, float* dcond, hipStream_t s, bool pairs = false, int nv = 0) {
    INBwdArgs a;
    a.g = g; a.y = y; a.mean = stats; a.rstd = stats + (long)Bn * C;
    a.cond = cond; a.cond_sb = cond_sb; a.cond_off = cond_off;
    a.dy = dy; a.dcond = dcond; a.dcond_sb = cond_sb; a.dcond_off = cond_off;
    a.R = Bn * C; a.C = C; a.T = T; a.relu = 1; a.slope = slope; a.planar = 0; a.nv_hint = nv;
    if (pairs) {
        a.R = Bn * (C / 2);
        return avc_launch_in_bwd_pairs(a, s);
    }
    return avc_launch_in_bwd(a, s);
}

// --------------------------------------------------------------------------
// forward
// --------------------------------------------------------------------------
static int enc_front(const avc_plan* p, const EncNet& e, const float* params, float* ws, const float* x, long sxb,
                     long sxc, int sxt, hipStream_t s) {
    // conv_bank (model.py:85-91): all bank members in ONE grouped launch writing the concat buffer in place
    const int B = p->B, T0 = e.T[0];
    const float SL = e.slope;
    const bool bh = p->bh;
    const long CCr = bh ? e.CC / 2 : e.CC, Cbr = bh ? e.c.c_bank / 2 : e.c.c_bank;   // rows per sample: pair rows with bh
    float* tail = ws + e.cat + (long)e.nb * Cbr * T0;   // raw input last (model.py:90)
    if (bh) RUN(avc_launch_to_pairs(x, sxb, sxc, sxt, B, e.c.c_in, T0, tail, CCr * T0, T0, s));   // ... as bf16 pairs, and the bank reads THAT copy
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.x.ptr = x; a.x.sb = sxb; a.x.sc = sxc; a.x.st = sxt; a.x.ps = 1;
    if (bh) { a.x.ptr = tail; a.x.sb = CCr * T0; a.x.sc = T0; a.x.st = 1; }
    a.B = B; a.Cred = bh ? e.c.c_in / 2 : e.c.c_in; a.Tsrc = T0;
    a.mode = 0; a.stride = 1; a.bf16 = p->compute;
    a.M = e.c.c_bank; a.Mp = avc_cdiv(e.c.c_bank, 128) * 128; a.Tout = T0;
    a.ob = CCr * T0; a.oc = T0; a.ot = 1; a.ops = 1;
    a.act = 1;
    a.slope = SL;
    a.ngroups = e.nb;
    a.img = bh ? AVC_IMG_K4H : AVC_IMG_K4;
    a.pairs = bh ? 1 : 0;
    for (int g = 0; g < e.nb; ++g) {
        const LayerP& L = p->layers[e.bank[g]];
        set_group(a.g[g], ws + L.wpf, p->par(params, L.b[0]), L.KS, L.CK, L.nchunk_f);
        a.g[g].out = ws + e.cat + (long)g * Cbr * T0;
    }
    RUN(avc_launch_conv(a, s, 0, p->tun));
    if (!bh) RUN(avc_launch_copy_rows(x, sxb, sxc, sxt, B, e.c.c_in, T0, tail, (long)e.CC * T0, T0, s));
    return 0;
}

static bool side_ready(const avc_plan* p);
static int pack_all(const avc_plan* p, const float* params, float* ws, hipStream_t s) {
    if (p->pack_tab_dev && !(p->tun.dbg_streams & 16)) {   // (bit 16, diagnostic: the per-image gather kernels the table launch is tested against)
        // ONE launch on the caller's stream.  (Round 4 ran the tail of the table on a helper stream under the next step's bank convs:
        // measured neutral -- 6.000 vs 6.009 ms/step -- and its read of `params` was ordered only against a later forward of the SAME
        // plan, a formal read / write race with an optimizer step or a parameter write that follows on another plan; removed.)
        return avc_launch_pack_table(p->pack_tab_dev, p->pack_blk_dev, p->pack_nblk, p->pack_tab_bytes, params, ws, s);
    }
    std::vector<PackArgs> all;
    for (size_t i = 0; i < p->layers.size(); ++i)
        if (p->layers[i].wpf >= 0 || p->layers[i].wpd >= 0) pack_layer(p, p->layers[i], params, ws, all);
    return avc_launch_pack_batch(all.data(), (int)all.size(), s);
}

// Weights -> LDS-image order for every layer of the plan, ONE launch.  A training loop calls this right behind the optimizer step
// (Solver.ae_step) and passes AVC_FWD_WEIGHTS_PACKED to the next avc_forward_ex: the step then opens with its first convolution.
extern "C" int avc_plan_pack_weights(const avc_plan* p, const float* params, float* ws, void* stream) {
    if (!p || !params || !ws) return fail(-1, "avc_plan_pack_weights: null argument");
    RUN(pack_all(p, params, ws, (hipStream_t)stream));
    return 0;
}

// din: the decoder's inputs of a decoder part plan (NULL: z = the reparameterised latent, emb = the speaker encoder's, both in ws)
static int forward_impl(const avc_plan* p, const float* params, const float* x, long sxb, long sxc, int sxt,
                        const float* xc, long scb, long scc, int sct, const float* eps, float* ws, hipStream_t s, bool packed = false,
                        const DecIn* din = nullptr) {
    const int B = p->B;
    const bool bh = p->bh;
    const int NV = (int)p->tun.in_pairs_nv;
    // 0. weights -> LDS-image order (they change every optimizer step): one launch, unless the caller packed them behind its
    // optimizer step already (AVC_FWD_WEIGHTS_PACKED)
    if (!packed) RUN(pack_all(p, params, ws, s));

    // part plans run one network: SpeakerEncoder.forward (AE.get_speaker_embeddings, model.py:393-395), ContentEncoder.forward or
    // Decoder.forward (model.py:265-277 / 301-323 / 347-371) -- the same launches as the whole plan's branch
    const bool do_spk = has_spk(p->flags), do_enc = has_enc(p->flags), do_dec = has_dec(p->flags);
    // first kernels of the content encoder (conv bank, in_conv, InstanceNorm) on the caller's stream
    auto content_front = [&]() -> int {
        if (!do_enc) return 0;
        const EncNet& e = p->enc;
        const float SL = e.slope;
        const int Cc = e.c.c_h;
        const long C = bh ? Cc / 2 : Cc, CCr = bh ? e.CC / 2 : e.CC;
        RUN(enc_front(p, e, params, ws, x, sxb, sxc, sxt, s));
        ConvArgs a = mk_fwd(p, SL, p->layers[e.in_conv], params, ws, ws + e.cat, CCr * e.T[0], e.T[0], 1, B, e.T[0], ws + e.h0, (long)C * e.T[0], e.T[0], 1, 0);
        RUN(conv_in_fwd(p, a, SL, B, Cc, e.T[0], nullptr, 0, 0, nullptr, 0, 0, ws + e.out[0], ws + e.st0, s, 0, 0, bh, 0, NV));
        return 0;
    };
    // ---------------- speaker encoder (model.py:265-277), concurrent with the content encoder
    const hipStream_t mainS = s;
    const hipStream_t sideS = do_spk ? fork_side(p, mainS) : mainS;
    if (!do_spk) RUN(content_front());
    if (do_spk) {
        const hipStream_t s = sideS;
        const EncNet& e = p->spk;
        const float SL = e.slope;
        const int Cc = e.c.c_h;                       // channels
        const long C = bh ? Cc / 2 : Cc;              // rows per sample of a [B, c_h, T] tensor (pair rows with bh): every stride below
        const long CCr = bh ? e.CC / 2 : e.CC;
        RUN(enc_front(p, e, params, ws, xc, scb, scc, sct, s));
        RUN(content_front());   // (main stream) issued under this branch's long bank kernel: the content encoder is the longer branch
        {
            const LayerP& L = p->layers[e.in_conv];
            ConvArgs a = mk_fwd(p, SL, L, params, ws, ws + e.cat, CCr * e.T[0], e.T[0], 1, B, e.T[0], ws + e.h0, (long)C * e.T[0], e.T[0], 1, 1);
            RUN(avc_launch_conv(a, s, 0, p->tun));
        }
        for (int l = 0; l < e.n; ++l) {
            const int Ti = e.T[l], To = e.T[l + 1];
            ConvArgs a = mk_fwd(p, SL, p->layers[e.c1[l]], params, ws, ws + e.out[l], (long)C * Ti, Ti, 1, B, Ti, ws + e.a1[l], (long)C * Ti, Ti, 1, 1);
            RUN(avc_launch_conv(a, s, 0, p->tun));
            ConvArgs b = mk_fwd(p, SL, p->layers[e.c2[l]], params, ws, ws + e.a1[l], (long)C * Ti, Ti, 1, B, Ti, ws + e.a2[l], (long)C * To, To, 1, 1);
            b.g[0].out2 = ws + e.out[l + 1];
            set_res(b, ws + e.out[l], e.c.subsample[l] > 1 ? AVC_RES_AVGPOOL2 : AVC_RES_IDENTITY, (long)C * Ti, Ti, 1, Ti);
            RUN(avc_launch_conv(b, s, 0, p->tun));
        }
        const int Tn = e.T[e.n];
        if (bh) RUN(avc_launch_timepool_fwd_pairs(ws + e.out[e.n], B, Cc, Tn, ws + e.pooled, s));
        else RUN(avc_launch_timepool_fwd(ws + e.out[e.n], B, Cc, Tn, ws + e.pooled, s));
        // dense blocks + output layer: ONE fused launch (dense.hip); activations channel-major [C][B]
        {
            DenseArgs da = dense_stack_args(p, e, params, ws, false);
            da.in = ws + e.hd[0];
            da.emb = ws + p->emb;
            for (int l = 0; l < e.nd; ++l) da.layer[2 * l + 1].out2 = ws + e.hd[l + 1];   // (the second Linear of a block also stores h_{l+1})
            RUN(avc_launch_dense(da, 0, s));
        }
    }

    // ---------------- content encoder (model.py:301-323)
    if (do_enc) {
        const EncNet& e = p->enc;
        const float SL = e.slope;
        const int Cc = e.c.c_h;
        const long C = bh ? Cc / 2 : Cc, CCr = bh ? e.CC / 2 : e.CC;
        // (conv bank, in_conv and its InstanceNorm were issued by content_front(), above)
        for (int l = 0; l < e.n; ++l) {
            const int Ti = e.T[l], To = e.T[l + 1];
            ConvArgs a = mk_fwd(p, SL, p->layers[e.c1[l]], params, ws, ws + e.out[l], (long)C * Ti, Ti, 1, B, Ti, ws + e.y1[l], (long)C * Ti, Ti, 1, 0);
            RUN(conv_in_fwd(p, a, SL, B, Cc, Ti, nullptr, 0, 0, nullptr, 0, 0, ws + e.a1[l], ws + e.st1[l], s, 0, 0, bh, 0, NV));
            ConvArgs b = mk_fwd(p, SL, p->layers[e.c2[l]], params, ws, ws + e.a1[l], (long)C * Ti, Ti, 1, B, Ti, ws + e.y2[l], (long)C * To, To, 1, 0);
            const int rmode = e.c.subsample[l] > 1 ? AVC_RES_AVGPOOL2 : AVC_RES_IDENTITY;
            RUN(conv_in_fwd(p, b, SL, B, Cc, To, nullptr, 0, 0, ws + e.out[l], rmode, Ti, ws + e.out[l + 1], ws + e.st2[l], s, 0, 0, bh, 0, NV));
        }
        const int Tb = p->Tb;
        ConvArgs h = mk_fwd(p, SL, p->layers[e.heads], params, ws, ws + e.out[e.n], (long)C * Tb, Tb, 1, B, Tb, ws + p->muls, (long)2 * e.c.c_out * Tb, Tb, 1, 0);
        h.pairs = 0;   // mu | log_sigma stay fp32 (the loss and the reparameterisation read them)
        RUN(avc_launch_conv(h, s, 0, p->tun));
    }

    join_side(p, mainS, sideS);
    // ---------------- reparameterisation (model.py:383-384) + decoder (model.py:347-371)
    if (do_dec) {
        const DecNet& d = p->dec;
        const float SL = d.slope;
        const int Cc = d.c.c_h, Czc = d.c.c_in, Tb = p->Tb;
        const long C = bh ? Cc / 2 : Cc, Cz = bh ? Czc / 2 : Czc;   // rows per sample (pair rows with bh)
        // z and emb: the workspace's own, or a decoder part plan's caller tensors read in place (pair plans: z converted to pairs first)
        const float* zs = ws + d.z;
        long zsb = Cz * Tb, zsc = Tb;
        int zst = 1;
        if (din && !bh) {
            zs = din->z; zsb = din->szb; zsc = din->szc; zst = din->szt;
        } else if (din) {
            RUN(avc_launch_to_pairs(din->z, din->szb, din->szc, din->szt, B, Czc, Tb, ws + d.z, Cz * Tb, Tb, s));
        } else if (bh) {
            RUN(avc_launch_reparam_fwd_pairs(ws + p->muls, eps, B, Czc, Tb, ws + d.z, s));
        } else {
            RUN(avc_launch_reparam_fwd(ws + p->muls, eps, B, Czc, Tb, ws + d.z, s));
        }
        const float* es = din ? din->emb : ws + p->emb;
        const long esb = din ? din->seb : d.c.c_cond, esc = din ? din->sec : 1;
        const long csb = (long)2 * d.n * 2 * Cc;
        {   // all 2n AdaIN affine Linears as ONE GEMM on emb (they share their input)
            ConvArgs a = mk_fwd(p, SL, p->layers[d.affine], params, ws, es, 0, esc, (int)esb, 1, B, ws + d.cond, 0, 1, (int)csb, 0);
            RUN(avc_launch_conv(a, s, 0, p->tun));
        }
        // The decoder is one serial chain of ~40 small kernels (T_l = 16..128): alone on the GPU it leaves
        // most CUs waiting on launch / pipeline latency (0.86 ms with one kernel in flight, traced).  Two
        // half-batch chains on two streams interleave their phases; every tensor is [B, ...], so a half is
        // a pointer offset.
        // phase 0: in_conv + IN; phases 1 .. 2n: (first conv + AdaIN) / (second conv + AdaIN + residual) of block (ph - 1) / 2; phase 2n + 1: out_conv
        auto dec_phase = [&](int b0, int Bn, hipStream_t s, int ph) -> int {
            const long ob0 = (long)b0 * C * Tb;
            const float* cond = ws + d.cond + (long)b0 * csb;
            if (ph == 0) {
                ConvArgs a = mk_fwd(p, SL, p->layers[d.in_conv], params, ws, zs + (long)b0 * zsb, zsb, zsc, zst, Bn, Tb, ws + d.y0 + ob0, (long)C * Tb, Tb, 1, 0);
                RUN(conv_in_fwd(p, a, SL, Bn, Cc, Tb, nullptr, 0, 0, nullptr, 0, 0, ws + d.out[0] + ob0, ws + d.st0, s, B, b0, bh, 0, NV));
                return 0;
            }
            if (ph == 2 * d.n + 1) {
                const int To = p->Tout;
                ConvArgs o = mk_fwd(p, SL, p->layers[d.out_conv], params, ws, ws + d.out[d.n] + (long)b0 * C * To, (long)C * To, To, 1, Bn, To,
                                    ws + p->decb + (long)b0 * p->M * To, (long)p->M * To, To, 1, 0);
                o.pairs = 0;   // dec is fp32 (the L1 loss / the caller read it)
                RUN(avc_launch_conv(o, s, 0, p->tun));
                return 0;
            }
            const int l = (ph - 1) / 2;
            const int Ti = d.T[l], To = d.T[l + 1], up = d.c.upsample[l];
            const long oi = (long)b0 * C * Ti, oo = (long)b0 * C * To;
            if ((ph - 1) % 2 == 0) {
                ConvArgs a = mk_fwd(p, SL, p->layers[d.c1[l]], params, ws, ws + d.out[l] + oi, (long)C * Ti, Ti, 1, Bn, Ti, ws + d.y1[l] + oi, (long)C * Ti, Ti, 1, 0);
                RUN(conv_in_fwd(p, a, SL, Bn, Cc, Ti, cond, csb, (2 * l) * 2 * Cc, nullptr, 0, 0, ws + d.a1[l] + oi, ws + d.st1[l], s, B, b0, bh, 0, NV));
                return 0;
            }
            // second conv: C*up channels, pixel-shuffled on store into [B, C, Ti*up]  (model.py:359-361)
            ConvArgs b = mk_fwd(p, SL, p->layers[d.c2[l]], params, ws, ws + d.a1[l] + oi, (long)C * Ti, Ti, 1, Bn, Ti, ws + d.y2[l] + oo, (long)C * To, To, 1, 0);
            b.ops = up;
            if (bh) {   // the conv-output pairs [B][c_h up / 2][Ti] ARE the natural bf16 rows of the shuffled tensor: "planar" y2 (rowops_pairs.hip)
                b.ops = 1;
                b.ob = (long)C * To; b.oc = Ti;
            }
            RUN(conv_in_fwd(p, b, SL, Bn, Cc, To, cond, csb, (2 * l + 1) * 2 * Cc, ws + d.out[l] + oi, up > 1 ? AVC_RES_UP2 : AVC_RES_IDENTITY, Ti,
                            ws + d.out[l + 1] + oo, ws + d.st2[l], s, B, b0, bh, (bh && up > 1) ? 1 : 0, NV));
            return 0;
        };
        const int nph = 2 * d.n + 2;
        if (B >= p->tun.dec_split_min && side_ready(p)) {
            // the host ISSUES the two chains phase by phase in turn: a chain issued whole before the other one starts has run to its end by the
            // time the second chain's first launch reaches the GPU (the kernels are as short as a launch call: traced, profiles/r03_bf16s_timeline.txt)
            const int Bh = B / 2;
            const hipStream_t s2 = fork_side(p, s);
            for (int ph = 0; ph < nph; ++ph) {
                RUN(dec_phase(0, Bh, s, ph));
                RUN(dec_phase(Bh, B - Bh, s2, ph));
            }
            join_side(p, s, s2);
        } else {
            for (int ph = 0; ph < nph; ++ph) RUN(dec_phase(0, B, s, ph));
        }
    }
    return 0;
}

extern "C" int avc_forward(const avc_plan* p, const float* params, const float* x, long sxb, long sxc, int sxt,
                           const float* x_cond, long scb, long scc, int sct, const float* eps, float* ws, void* stream) {
    if (!p || !params || !x || !ws) return fail(-1, "avc_forward: null argument");
    if (p->flags & AVC_PLAN_RAGGED) return fail(-8, "avc_forward: ragged plans run through avc_forward_ragged");
    if (p->flags & AVC_PLAN_DECODER_ONLY) return fail(-8, "avc_forward: decoder part plans run through avc_decoder_forward");
    if (!x_cond) {
        x_cond = x; scb = sxb; scc = sxc; sct = sxt;
    }
    return forward_impl(p, params, x, sxb, sxc, sxt, x_cond, scb, scc, sct, eps, ws, (hipStream_t)stream);
}

extern "C" int avc_forward_ex(const avc_plan* p, const float* params, const float* x, long sxb, long sxc, int sxt,
                              const float* x_cond, long scb, long scc, int sct, const float* eps, float* ws, int flags, void* stream) {
    if (!p || !params || !x || !ws) return fail(-1, "avc_forward_ex: null argument");
    if (p->flags & AVC_PLAN_RAGGED) return fail(-8, "avc_forward_ex: ragged plans run through avc_forward_ragged");
    if (p->flags & AVC_PLAN_DECODER_ONLY) return fail(-8, "avc_forward_ex: decoder part plans run through avc_decoder_forward");
    if (flags & ~AVC_FWD_WEIGHTS_PACKED) return fail(-1, "avc_forward_ex: unknown flag");
    if (!x_cond) {
        x_cond = x; scb = sxb; scc = sxc; sct = sxt;
    }
    return forward_impl(p, params, x, sxb, sxc, sxt, x_cond, scb, scc, sct, eps, ws, (hipStream_t)stream, (flags & AVC_FWD_WEIGHTS_PACKED) != 0);
}

// Decoder.forward(z, cond) (model.py:347-371) on a decoder part plan: the caller's z / emb in place of the latent and the embedding
extern "C" int avc_decoder_forward(const avc_plan* p, const float* params, const float* z, long szb, long szc, int szt, const float* emb,
                                   long seb, long sec, float* ws, int flags, void* stream) {
    if (!p || !params || !z || !emb || !ws) return fail(-1, "avc_decoder_forward: null argument");
    if (!(p->flags & AVC_PLAN_DECODER_ONLY)) return fail(-8, "avc_decoder_forward: the plan was not created with AVC_PLAN_DECODER_ONLY");
    if (p->flags & AVC_PLAN_RAGGED) return fail(-8, "avc_decoder_forward: ragged decoder plans run through avc_decoder_forward_ragged");
    if (flags & ~AVC_FWD_WEIGHTS_PACKED) return fail(-1, "avc_decoder_forward: unknown flag");
    const DecIn din = {z, szb, szc, szt, emb, seb, sec};
    return forward_impl(p, params, nullptr, 0, 0, 0, nullptr, 0, 0, 0, nullptr, ws, (hipStream_t)stream, (flags & AVC_FWD_WEIGHTS_PACKED) != 0,
                        &din);
}

extern "C" int avc_loss(const avc_plan* p, const float* x, long sxb, long sxc, int sxt, float lambda_rec, float* ws,
                        void* stream) {
    if (!p) return fail(-1, "avc_loss: null plan");
    if (p->flags & AVC_PLAN_PARTS) return fail(-8, "avc_loss: part plans have no loss (the caller's autograd takes the losses of solver.py:84-88)");
    if (p->flags & AVC_PLAN_INFERENCE) return fail(-8, "avc_loss: the plan was created with AVC_PLAN_INFERENCE");
    if (p->Tout != p->T) return fail(-7, "avc_loss: L1Loss needs dec and x of equal length (T % 8 == 0 for the stock config)");
    RUN(avc_launch_loss(ws + p->decb, x, sxb, sxc, sxt, p->B, p->M, p->T, ws + p->muls, p->dec.c.c_in, p->Tb, lambda_rec,
                        ws + p->ddec, ws + p->loss_partial, ws + p->losses, (hipStream_t)stream));
    return 0;
}

// --------------------------------------------------------------------------
// backward
// --------------------------------------------------------------------------
static int enc_back_front(BwdCtx& c, const EncNet& e, const float* x, long sxb, long sxc, int sxt, const float* dy_in) {
    // dy_in: gradient wrt the in_conv output [B, C, T0]
    const avc_plan* p = c.p;
    const bool bh = p->bh;
    const int B = p->B, T0 = e.T[0];
    const long C = bh ? e.c.c_h / 2 : e.c.c_h, CCr = bh ? e.CC / 2 : e.CC, Cbr = bh ? e.c.c_bank / 2 : e.c.c_bank;   // rows per sample (pair rows with bh)
    const float SL = e.slope;
    float* ws = c.ws;
    const LayerP& L = p->layers[e.in_conv];
    RUN(wgrad_layer(c, L, ws + e.cat, CCr * T0, T0, 1, dy_in, (long)C * T0, T0, 1, 1, B, T0, T0));
    if (!c.dry) {
        // d(cat) for the bank channels only, masked by the bank ReLU (cat > 0)
        ConvArgs a = mk_dgrad(SL, L, ws, dy_in, (long)C * T0, T0, 1, 1, B, T0, T0, nullptr, CCr * T0, T0, 1);
        a.g[0].out2 = ws + e.dcat;
        a.g[0].mask = ws + e.cat;
        RUN(avc_launch_conv(a, c.s, 0, p->tun));
    }
    if (!c.dry && e.in_pass >= 0) {
        // AVC_PLAN_INPUT_GRADS: d(x) = W_in[:, nb c_bank:]^T dy_in + sum_g bank_g^T(dcat_g), one implicit-GEMM input-gradient launch per
        // term, each adding the previous partial sum (the residual join of its epilogue, in place) -- a fixed order, no atomics.  The
        // reflect-pad adjoint of every bank width is folded into the launch's fetch (mirror windows).  fp32 output in every mode.
        const long M = e.c.c_in;
        float* dx = ws + e.dx;
        ConvArgs a = mk_dgrad(SL, p->layers[e.in_pass], ws, dy_in, (long)C * T0, T0, 1, 1, B, T0, T0, dx, M * T0, T0, 1);
        a.pairs = 0;
        RUN(avc_launch_conv(a, c.s, 0, p->tun));
        for (int g = 0; g < e.nb; ++g) {
            ConvArgs b = mk_dgrad(SL, p->layers[e.bank[g]], ws, ws + e.dcat + (long)g * Cbr * T0, CCr * T0, T0, 1, 1, B, T0, T0, dx, M * T0, T0, 1);
            b.pairs = 0;
            set_res(b, dx, AVC_RES_IDENTITY, M * T0, T0, 1, T0);
            RUN(avc_launch_conv(b, c.s, 0, p->tun));
        }
    }
    for (int g = 0; g < e.nb; ++g) {
        const LayerP& Lb = p->layers[e.bank[g]];
        if (bh)   // the bank read the pair copy of the input at the tail of the concat buffer
            RUN(wgrad_layer(c, Lb, ws + e.cat + (long)e.nb * Cbr * T0, CCr * T0, T0, 1, ws + e.dcat + (long)g * Cbr * T0, CCr * T0, T0, 1, 1, B, T0, T0));
        else
            RUN(wgrad_layer(c, Lb, x, sxb, sxc, sxt, ws + e.dcat + (long)g * e.c.c_bank * T0, (long)e.CC * T0, T0, 1, 1, B, T0, T0));
    }
    return 0;
}

int avc_backward_impl(const avc_plan* p, const float* params, const float* x, long sxb, long sxc, int sxt, const float* xc,
                      long scb, long scc, int sct, const float* eps, const float* d_dec, const float* d_muls_up,
                      const float* d_emb_up, float lambda_kl, float* grads, float* ws, hipStream_t s, bool dry,
                      long* slab_need, const DecIn* din) {
    BwdCtx c;
    c.p = p; c.params = params; c.grads = grads; c.ws = ws; c.s = s; c.dry = dry; c.slab_used = 0;
    if (!dry) avc_prof_mark(0, s);
    c.nev = 0; c.dy_used = 0; c.pend_units = 0;
    const bool overlap = !dry && side_ready(p) && !(p->tun.dbg_streams & 1);
    const bool use_side = !dry && !(p->tun.dbg_streams & 2);
    c.wstream = overlap ? p->wstream[0] : s;
    const int B = p->B;
    const bool bh = p->bh;
    const int NV = (int)p->tun.in_pairs_nv;
    float* gA = ws + p->gA;
    float* gB = ws + p->gB;
    float* gC = ws + p->gC;
    float* dyA = nullptr;
    float* dyB = nullptr;
    auto rot = [&]() { float* t = gA; gA = gC; gC = t; };
    // part plans: one network's backward (a decoder part plan's z / emb are the caller's: din)
    const bool do_spk = has_spk(p->flags), do_enc = has_enc(p->flags), do_dec = has_dec(p->flags);
    const bool dec_only = (p->flags & AVC_PLAN_DECODER_ONLY) != 0;

    // ---------------- decoder
    if (do_dec) {
        const DecNet& d = p->dec;
        const float SL = d.slope;
        const int Cc = d.c.c_h, Czc = d.c.c_in, Tb = p->Tb, To = p->Tout;
        const long C = bh ? Cc / 2 : Cc, Cz = bh ? Czc / 2 : Czc;   // rows per sample (pair rows with bh): every stride / offset below
        const long Mr = bh ? p->M / 2 : p->M;
        const long csb = (long)2 * d.n * 2 * Cc;
        const float* ddec = d_dec ? d_dec : ws + p->ddec;
        // the in_conv's input z and the affine GEMM's input emb, as the forward pass read them
        const float* zs = ws + d.z;
        long zsb = Cz * Tb, zsc = Tb;
        int zst = 1;
        if (din && !bh) { zs = din->z; zsb = din->szb; zsc = din->szc; zst = din->szt; }
        const float* es = din ? din->emb : ws + p->emb;
        const long esb = din ? din->seb : d.c.c_cond, esc = din ? din->sec : 1;
        if (bh) {   // the conv launches read pair operands: d(dec) (fp32: written by avc_loss or handed in by the autograd seam) -> pairs
            if (!dry) RUN(avc_launch_to_pairs(ddec, (long)p->M * To, To, 1, B, p->M, To, ws + p->ddecp, Mr * To, To, s));
            ddec = ws + p->ddecp;
        }
        const LayerP& Lo = p->layers[d.out_conv];
        const LayerP& Li = p->layers[d.in_conv];
        // every dy a weight-gradient launch reads gets its own buffer (the launches run later, beside the encoders' backward)
        float* dy2[AVC_MAX_BLOCKS];
        float* dy1[AVC_MAX_BLOCKS];
        for (int l = d.n - 1; l >= 0; --l) {
            dy2[l] = c.fresh((long)B * C * d.T[l + 1]);
            dy1[l] = c.fresh((long)B * C * d.T[l]);
        }
        float* dy0 = c.fresh((long)B * C * Tb);
        // The decoder's backward is one serial chain of ~26 small kernels (T_l = 128 .. 16) that runs ALONE on the GPU -- nothing
        // else is ready before d(emb) and d(muls) exist (traced: 0.7 ms with one kernel in flight).  Like the forward pass it is
        // issued as two half-batch chains on two streams for B >= dec_split_min: every tensor is [B, ...], a half is a pointer
        // offset, and InstanceNorm / AdaIN statistics and d(cond) rows are per sample.
        struct ChainSt {
            float *gA, *gB, *gC;
            bool fused;   // the InstanceNorm backward that opens the NEXT phase already ran inside this phase's input-gradient launch
        };
        // phase 0: out_conv input gradient; phases 1 .. 2n walk the blocks from the last one: (AdaIN backward of the second conv + its input
        // gradient) / (AdaIN backward of the first conv + its input gradient joined with the skip path); phase 2n + 1: IN backward + in_conv
        auto chain_phase = [&](ChainSt& st, int b0, int Bn, hipStream_t s, int ph) -> int {
            auto half_in_bwd = [&](const float* g, long off, long yoff, long stoff, int T, int coff, bool cond, float* dy, int planar = 0) -> int {
                INBwdArgs a;
                a.g = g + off; a.y = ws + yoff + off;
                a.mean = ws + stoff + (long)b0 * Cc; a.rstd = ws + stoff + (long)B * Cc + (long)b0 * Cc;
                a.cond = cond ? ws + d.cond + (long)b0 * csb : nullptr; a.cond_sb = csb; a.cond_off = coff;
                a.dy = dy + off; a.dcond = cond ? ws + d.dcond + (long)b0 * csb : nullptr; a.dcond_sb = csb; a.dcond_off = coff;
                a.R = Bn * Cc; a.C = Cc; a.T = T; a.relu = 1; a.slope = SL; a.planar = planar; a.nv_hint = (int)p->tun.in_pairs_nv;
                if (bh) {
                    a.R = Bn * (Cc / 2);
                    return avc_launch_in_bwd_pairs(a, s);
                }
                return avc_launch_in_bwd(a, s);
            };
            // An input-gradient launch whose output rows are the d(out) of the NEXT phase's InstanceNorm layer runs that layer's backward
            // in its epilogue where the tile holds whole rows (rows of 16 / 32 / 64 frames, fp32: avc_conv_inb_fusable); the next phase
            // then skips its row kernel.  `keep_g`: the launch's own output is read again (the block's skip path).
            auto dgrad_inb = [&](ConvArgs& a, bool keep_g, long off, long yoff, long stoff, int T, int coff, bool cond, float* dy, bool planar = false) -> int {
                st.fused = false;
                if (!planar && a.Tout == T && avc_conv_inb_fusable(a, p->tun)) {   // (pair tensors too since round 6; the "planar" rows behind a pixel shuffle keep the row kernel)
                    a.inb.dy = dy + off; a.inb.y = ws + yoff + off;
                    a.inb.mean = ws + stoff + (long)b0 * Cc; a.inb.rstd = ws + stoff + (long)B * Cc + (long)b0 * Cc;
                    a.inb.cond = cond ? ws + d.cond + (long)b0 * csb : nullptr; a.inb.cond_sb = csb; a.inb.cond_off = coff;
                    a.inb.dcond = cond ? ws + d.dcond + (long)b0 * csb : nullptr; a.inb.dcond_sb = csb; a.inb.dcond_off = coff;
                    a.inb.C = Cc; a.inb.relu = 1;
                    if (!keep_g) a.g[0].out = nullptr;
                    st.fused = true;
                }
                return avc_launch_conv(a, s, 0, p->tun);
            };
            const bool was_fused = st.fused;   // (set by the previous phase of THIS chain)
            if (ph == 0) {
                const long oi = (long)b0 * Mr * To, oo = (long)b0 * C * To;
                ConvArgs a = mk_dgrad(SL, Lo, ws, ddec + oi, Mr * To, To, 1, 1, Bn, To, To, st.gA + oo, (long)C * To, To, 1);
                // next: the AdaIN backward of the last block's second conv (rows of To frames)
                const int ln = d.n - 1;
                RUN(dgrad_inb(a, true, oo, d.y2[ln], d.st2[ln], d.T[ln + 1], (2 * ln + 1) * 2 * Cc, true, dy2[ln], bh && d.c.upsample[ln] > 1));
                return 0;
            }
            if (ph == 2 * d.n + 1) {
                const long ob = (long)b0 * C * Tb;
                if (!was_fused) RUN(half_in_bwd(st.gA, ob, d.y0, d.st0, Tb, 0, false, dy0));
                st.fused = false;
                ConvArgs a = mk_dgrad(SL, Li, ws, dy0 + ob, (long)C * Tb, Tb, 1, 1, Bn, Tb, Tb, ws + p->dz + (long)b0 * Czc * Tb, (long)Czc * Tb, Tb, 1);
                a.pairs = 0;   // d(z) is fp32: the latent backward combines it with the fp32 mu / log_sigma
                RUN(avc_launch_conv(a, s, 0, p->tun));
                return 0;
            }
            const int l = d.n - 1 - (ph - 1) / 2;
            const int Ti = d.T[l], T2 = d.T[l + 1], up = d.c.upsample[l];
            const long o2 = (long)b0 * C * T2, o1 = (long)b0 * C * Ti;
            if ((ph - 1) % 2 == 0) {
                if (!was_fused) RUN(half_in_bwd(st.gA, o2, d.y2[l], d.st2[l], T2, (2 * l + 1) * 2 * Cc, true, dy2[l], (bh && up > 1) ? 1 : 0));
                // dy2 is the pixel-shuffled layout [B, C, Ti*up]; view it as the conv output [B, C*up, Ti]
                // (pair plans: dy2 was written planar = as the conv-output pairs [B][c_h up / 2][Ti], a plain stride-1 source)
                ConvArgs a = bh ? mk_dgrad(SL, p->layers[d.c2[l]], ws, dy2[l] + o2, (long)C * T2, Ti, 1, 1, Bn, Ti, Ti, st.gB + o1, (long)C * Ti, Ti, 1)
                                : mk_dgrad(SL, p->layers[d.c2[l]], ws, dy2[l] + o2, (long)C * T2, T2, up, up, Bn, Ti, Ti, st.gB + o1, (long)C * Ti, Ti, 1);
                // next: the AdaIN backward of this block's first conv (rows of Ti frames); gB has no other reader
                RUN(dgrad_inb(a, false, o1, d.y1[l], d.st1[l], Ti, (2 * l) * 2 * Cc, true, dy1[l]));
                return 0;
            }
            if (!was_fused) RUN(half_in_bwd(st.gB, o1, d.y1[l], d.st1[l], Ti, (2 * l) * 2 * Cc, true, dy1[l]));
            ConvArgs a = mk_dgrad(SL, p->layers[d.c1[l]], ws, dy1[l] + o1, (long)C * Ti, Ti, 1, 1, Bn, Ti, Ti, st.gC + o1, (long)C * Ti, Ti, 1);
            set_res(a, st.gA + o2, up > 1 ? AVC_RES_UPT : AVC_RES_IDENTITY, (long)C * T2, T2, 1, T2);
            // next: the AdaIN backward of the previous block's second conv, or the in_conv's InstanceNorm (rows of Ti frames); gC feeds the skip path too
            if (l > 0) RUN(dgrad_inb(a, true, o1, d.y2[l - 1], d.st2[l - 1], Ti, (2 * (l - 1) + 1) * 2 * Cc, true, dy2[l - 1], bh && d.c.upsample[l - 1] > 1));
            else RUN(dgrad_inb(a, true, o1, d.y0, d.st0, Tb, 0, false, dy0));
            float* t = st.gA; st.gA = st.gC; st.gC = t;
            return 0;
        };
        // The weight gradient of a layer is RECORDED right behind the phase that produces its dy.  By default all of them are held and go
        // out behind the dense-stack backward kernel (below).  avc_tuning.dec_wgrad_flush = N > 0: every N recorded layers go out at once,
        // on the wgrad stream, as launches of only dec_wgrad_wgs persistent workgroups -- the decoder's backward chain is latency-bound
        // and leaves most CUs idle; a launch that occupies only part of the chip is filler for exactly that phase.
        c.hold = true;
        const int early = p->tun.dec_wgrad_flush;
        auto rec_phase = [&](int ph) -> int {   // (the order of the records is the order of round 3: out_conv, blocks n-1 .. 0 (second, first conv), in_conv)
            if (ph == 0) return wgrad_layer(c, Lo, ws + d.out[d.n], (long)C * To, To, 1, ddec, Mr * To, To, 1, 1, B, To, To);
            if (ph == 2 * d.n + 1) return wgrad_layer(c, Li, zs, zsb, zsc, zst, dy0, (long)C * Tb, Tb, 1, 1, B, Tb, Tb);
            const int l = d.n - 1 - (ph - 1) / 2;
            const int Ti = d.T[l], T2 = d.T[l + 1], up = d.c.upsample[l];
            if ((ph - 1) % 2 == 0) {
                if (bh) return wgrad_layer(c, p->layers[d.c2[l]], ws + d.a1[l], (long)C * Ti, Ti, 1, dy2[l], (long)C * T2, Ti, 1, 1, B, Ti, Ti);
                return wgrad_layer(c, p->layers[d.c2[l]], ws + d.a1[l], (long)C * Ti, Ti, 1, dy2[l], (long)C * T2, T2, up, up, B, Ti, Ti);
            }
            return wgrad_layer(c, p->layers[d.c1[l]], ws + d.out[l], (long)C * Ti, Ti, 1, dy1[l], (long)C * Ti, Ti, 1, 1, B, Ti, Ti);
        };
        {
            const int nph = 2 * d.n + 2;
            ChainSt st0 = {ws + p->gA, ws + p->gB, ws + p->gC, false}, st1 = st0;
            const bool split = use_side && B >= p->tun.dec_split_min && side_ready(p);
            const int Bh = B / 2;
            const hipStream_t s2 = split ? fork_side(p, s) : s;
            for (int ph = 0; ph < nph; ++ph) {   // the two half-batch chains are issued in turn (see the forward pass)
                if (!dry) {
                    if (split) {
                        RUN(chain_phase(st0, 0, Bh, s, ph));
                        RUN(chain_phase(st1, Bh, B - Bh, s2, ph));
                    } else {
                        RUN(chain_phase(st0, 0, B, s, ph));
                    }
                }
                // phase ph consumed (ph = 0: d(dec)) or produced (its InstanceNorm backward) the dy of this layer -- on BOTH chains' streams
                RUN(rec_phase(ph));
                if (early > 0 && (int)c.pend.size() >= early && ph + 1 < nph) {
                    c.s_extra = s2;
                    c.target_wgs = (int)p->tun.dec_wgrad_wgs;
                    RUN(flush_wgrads(c, true));
                    c.s_extra = nullptr;
                    c.target_wgs = 0;
                }
            }
            if (split) join_side(p, s, s2);
        }
        // affine Linears: dW/db from (emb, dcond), d(emb) = W^T dcond (+ upstream)
        const LayerP& La = p->layers[d.affine];
        RUN(wgrad_layer(c, La, es, 0, esc, (int)esb, ws + d.dcond, 0, 1, (int)csb, 1, 1, B, B));
        {
            // d(emb)[i][b] = sum_o W[o][i] * dcond[b][o]: a 128 x B output with K = 2n*2C = 3072.  As a dgrad
            // launch that is 8 workgroups walking 96 chunks one after the other (206 us on the critical
            // path, measured); as a split-K GEMM through the weight-gradient kernel ("co" = i read from the
            // packed forward image [i][o], "ci" = b read from dcond [b][o], "t" = o) it is ~50 workgroups.
            WgradArgs w;
            memset(&w, 0, sizeof(w));
            w.x.ptr = ws + d.dcond; w.x.sb = 0; w.x.sc = csb; w.x.st = 1; w.x.ps = 1;
            w.dy.ptr = ws + La.wplain; w.dy.sb = 0; w.dy.sc = La.Mp_f; w.dy.st = 1; w.dy.ps = 1;
            w.B = 1; w.Cin = B; w.Cout = d.c.c_cond; w.Tin = La.Cout; w.Tout = La.Cout;
            w.KS = 1; w.padL = 0; w.stride = 1; w.bf16 = bh ? AVC_COMPUTE_BF16 : p->compute;   // (fp32-stored operands either way)
            w.rows_per_src = w.Cout;
            avc_wgrad_plan_batch(&w, 1, 256);
            const long off = c.slab_used;
            c.slab_used += (w.slab_need + 63) / 64 * 64;
            if (!dry) {
                w.slab = ws + p->slab + off;
                w.dbslab = nullptr;
                w.dw = ws + p->demb;   // demb: channel-major [c_cond][B]
                w.db = nullptr;
                RUN(avc_launch_wgrad_batch(&w, 1, s, p->tun.wgrad_ablation));
                if (d_emb_up) RUN(avc_launch_add_transposed(ws + p->demb, d_emb_up, B, d.c.c_cond, s));
                if (dec_only) RUN(avc_launch_transpose(ws + p->demb_rm, ws + p->demb, d.c.c_cond, B, s));   // -> the caller's row-major [B, c_cond]
            }
        }
        if (dec_only) {   // no latent step and no speaker branch to hide the decoder's weight gradients under: they go out now
            c.hold = false;
            RUN(flush_wgrads(c));
            if (!dry && p->side_state == 1) hipEventRecord(p->ev_dec_grads, c.wstream);
        }
        // latent: KL term + reparameterisation (solver.py:86, model.py:384)
        if (!dry && !dec_only) {
            float lk = lambda_kl / (float)((long)B * Czc * Tb);
            RUN(avc_launch_latent_bwd(ws + p->muls, eps, ws + p->dz, d_muls_up, B, Czc, Tb, lk, ws + p->dmuls, s));
            if (bh) RUN(avc_launch_to_pairs(ws + p->dmuls, (long)2 * Czc * Tb, Tb, 1, B, 2 * Czc, Tb, ws + p->dmulsp, (long)Czc * Tb, Tb, s));
        }
        // (the decoder's weight gradients are launched from inside the speaker branch below, BEHIND the dense-stack backward kernel: that
        // kernel opens the speaker branch's critical chain, needs a whole CU's LDS per workgroup and cannot share a CU with a persistent
        // weight-gradient workgroup -- launched after 256 of those it waited for them: 413 instead of 66 us, traced in round 4)
    }

    // ---------------- content encoder (issued from inside the speaker branch below, right after that branch's first kernel: the host
    // issues launches about as fast as these kernels run, so whichever branch is issued second starts late by the other one's issue time)
    auto content_branch = [&]() -> int {
        const EncNet& e = p->enc;
        const float SL = e.slope;
        const int Cc = e.c.c_h, Tb = p->Tb;
        const long C = bh ? Cc / 2 : Cc, Co2 = bh ? e.c.c_out : 2 * e.c.c_out;   // rows per sample (pair rows with bh)
        const float* dmuls = ws + (bh ? p->dmulsp : p->dmuls);
        const LayerP& Lh = p->layers[e.heads];
        RUN(wgrad_layer(c, Lh, ws + e.out[e.n], (long)C * Tb, Tb, 1, dmuls, (long)Co2 * Tb, Tb, 1, 1, B, Tb, Tb));
        // An input-gradient launch whose output rows are the d(out) of the NEXT InstanceNorm layer runs that layer's backward in its
        // epilogue where the tile holds whole rows (avc_conv_inb_fusable); the row kernel then stays out of the chain.
        auto dgrad_inb = [&](ConvArgs& a, bool keep_g, const float* y, const float* st, int T, float* dy) -> bool {
            bool fused = false;
            if (a.Tout == T && avc_conv_inb_fusable(a, p->tun)) {   // (pair tensors too since round 6)
                a.inb.dy = dy; a.inb.y = y; a.inb.mean = st; a.inb.rstd = st + (long)B * Cc;
                a.inb.C = Cc; a.inb.relu = 1;
                if (!keep_g) a.g[0].out = nullptr;
                fused = true;
            }
            return fused;
        };
        bool fused = false;
        dyA = c.fresh((long)B * C * e.T[e.n]);   // d(y2) of the last block
        {
            ConvArgs a = mk_dgrad(SL, Lh, ws, dmuls, (long)Co2 * Tb, Tb, 1, 1, B, Tb, Tb, gA, (long)C * Tb, Tb, 1);
            fused = dgrad_inb(a, true, ws + e.y2[e.n - 1], ws + e.st2[e.n - 1], e.T[e.n], dyA);
            if (!dry) RUN(avc_launch_conv(a, s, 0, p->tun));
        }
        for (int l = e.n - 1; l >= 0; --l) {
            const int Ti = e.T[l], T2 = e.T[l + 1], sub = e.c.subsample[l];
            const LayerP& L1 = p->layers[e.c1[l]];
            const LayerP& L2 = p->layers[e.c2[l]];
            if (!dry && !fused) RUN(in_bwd(SL, gA, ws + e.y2[l], ws + e.st2[l], B, Cc, T2, nullptr, 0, 0, dyA, nullptr, s, bh, NV));
            dyB = c.fresh((long)B * C * Ti);
            {
                ConvArgs a = mk_dgrad(SL, L2, ws, dyA, (long)C * T2, T2, 1, 1, B, T2, Ti, gB, (long)C * Ti, Ti, 1);
                fused = dgrad_inb(a, false, ws + e.y1[l], ws + e.st1[l], Ti, dyB);   // gB has no other reader
                if (!dry) RUN(avc_launch_conv(a, s, 0, p->tun));
            }
            RUN(wgrad_layer(c, L2, ws + e.a1[l], (long)C * Ti, Ti, 1, dyA, (long)C * T2, T2, 1, 1, B, Ti, T2));
            if (!dry && !fused) RUN(in_bwd(SL, gB, ws + e.y1[l], ws + e.st1[l], B, Cc, Ti, nullptr, 0, 0, dyB, nullptr, s, bh, NV));
            dyA = c.fresh((long)B * C * Ti);   // d(y2) of block l - 1, or d(in_conv output) for l == 0: rows of Ti frames either way
            {
                ConvArgs a = mk_dgrad(SL, L1, ws, dyB, (long)C * Ti, Ti, 1, 1, B, Ti, Ti, gC, (long)C * Ti, Ti, 1);
                set_res(a, gA, sub > 1 ? AVC_RES_POOLT : AVC_RES_IDENTITY, (long)C * T2, T2, 1, T2);
                fused = dgrad_inb(a, true, l > 0 ? ws + e.y2[l - 1] : ws + e.h0, l > 0 ? ws + e.st2[l - 1] : ws + e.st0, Ti, dyA);   // gC feeds the skip path too
                if (!dry) RUN(avc_launch_conv(a, s, 0, p->tun));
            }
            RUN(wgrad_layer(c, L1, ws + e.out[l], (long)C * Ti, Ti, 1, dyB, (long)C * Ti, Ti, 1, 1, B, Ti, Ti));
            rot();
        }
        if (!dry && !fused) RUN(in_bwd(SL, gA, ws + e.h0, ws + e.st0, B, Cc, e.T[0], nullptr, 0, 0, dyA, nullptr, s, bh, NV));
        RUN(enc_back_front(c, e, x, sxb, sxc, sxt, dyA));
        if (!dry) avc_prof_mark(3, s);
        RUN(flush_wgrads(c));
        return 0;
    };

    if (!do_dec && do_enc && !dry) {   // content part plan: d(muls) = upstream + the KL term (solver.py:86), no z
        const int Czc = p->dec.c.c_in, Tb = p->Tb;
        float lk = lambda_kl / (float)((long)B * Czc * Tb);
        RUN(avc_launch_latent_bwd(ws + p->muls, nullptr, nullptr, d_muls_up, B, Czc, Tb, lk, ws + p->dmuls, s));
        if (bh) RUN(avc_launch_to_pairs(ws + p->dmuls, (long)2 * Czc * Tb, Tb, 1, B, 2 * Czc, Tb, ws + p->dmulsp, (long)Czc * Tb, Tb, s));
    }
    if (!do_dec && do_spk && !dry)   // speaker part plan: the caller's d(emb) [B, c_out] -> the dense stack's channel-major operand
        RUN(avc_launch_transpose(ws + p->demb, d_emb_up, B, p->spk.c.c_out, s));

    // ---------------- speaker encoder (side stream, own temporaries: concurrent with the content encoder)
    const hipStream_t mainS = s;
    const hipStream_t sideS = (use_side && do_spk) ? fork_side(p, mainS) : mainS;
    if (!do_spk && do_enc) {   // content part plan: its branch alone, on the caller's stream
        c.s = mainS;
        c.wstream = overlap ? p->wstream[0] : mainS;
        RUN(content_branch());
    }
    if (do_spk) {
        const hipStream_t s = sideS;
        c.s = sideS;
        float* gA = ws + p->gA2;
        float* gB = ws + p->gB2;
        float* gC = ws + p->gC2;
        float* dyA = nullptr;
        float* dyB = nullptr;
        c.wstream = (overlap && sideS != mainS) ? p->wstream[1] : sideS;
        auto rot = [&]() { float* t = gA; gA = gC; gC = t; };
        const EncNet& e = p->spk;
        const float SL = e.slope;
        const int Cc = e.c.c_h;
        const long C = bh ? Cc / 2 : Cc;   // rows per sample of the [B, c_h, T] tensors (pair rows with bh)
        float* dhA = ws + p->dhA;
        const LayerP& Lo = p->layers[e.outl];
        // output layer + dense blocks: ONE fused dgrad launch produces every dz (and d pooled);
        // the weight gradients are ordinary GEMMs over the batch on the wgrad stream
        {
            DenseArgs da = dense_stack_args(p, e, nullptr, ws, true);
            da.in = ws + p->demb;      // [c_out][B] channel-major (upstream d_emb is already folded into demb above: no in2)
            da.dpooled = dhA;
            float* dzl[AVC_DENSE_MAXL];
            for (int l = 0; l < da.nlayers; ++l) {
                const bool last = (l == da.nlayers - 1);
                dzl[l] = last ? nullptr : c.fresh((long)Cc * B);
                da.layer[l].dz = dzl[l];
            }
            if (!dry) RUN(avc_launch_dense(da, 1, s));
            if (!dry) avc_prof_mark(1, s);
            {   // the decoder's pending weight gradients: their dy operands are final on the main stream; they go out now, ordered behind
                // the dense-stack kernel as well
                const hipStream_t ws0 = overlap ? p->wstream[0] : mainS;
                if (overlap && sideS != mainS) {
                    hipEventRecord(p->ev_dense, sideS);
                    hipStreamWaitEvent(ws0, p->ev_dense, 0);
                }
                c.s = mainS;
                c.wstream = ws0;
                c.hold = false;
                RUN(flush_wgrads(c));  // decoder gradients are complete
                // ... which lets a data-parallel caller start their all-reduce under the encoders' backward
                // (avc_plan_stream_wait_grads): the decoder's parameters are the tail of the flat buffer
                if (!dry && p->side_state == 1) hipEventRecord(p->ev_dec_grads, c.wstream);
                if (!dry) avc_prof_mark(5, c.wstream);
                c.s = sideS;
                c.wstream = (overlap && sideS != mainS) ? p->wstream[1] : sideS;
            }
            const LayerP* gl[AVC_DENSE_MAXL];
            const float* gx[AVC_DENSE_MAXL];
            const float* gdy[AVC_DENSE_MAXL];
            int ng = 0;
            gl[ng] = &Lo; gx[ng] = ws + e.hd[e.nd]; gdy[ng] = ws + p->demb; ++ng;
            for (int l = e.nd - 1; l >= 0; --l) {
                gl[ng] = &p->layers[e.dn2[l]]; gx[ng] = ws + e.d1[l]; gdy[ng] = dzl[2 * l + 1]; ++ng;
                gl[ng] = &p->layers[e.dn1[l]]; gx[ng] = ws + e.hd[l]; gdy[ng] = dzl[2 * l]; ++ng;
            }
            // 13 Linear layers on [C][B] channel-major operands: same kernel instance -> ONE batched launch
            for (int i = 0; i < ng; ++i) RUN(wgrad_layer(c, *gl[i], gx[i], 0, B, 1, gdy[i], 0, B, 1, 1, 1, B, B));
        }
        // ... the content encoder's whole branch is issued now (main stream), under the dense-stack kernel that opens this branch
        RUN(flush_wgrads(c));
        c.s = mainS;
        c.wstream = overlap ? p->wstream[0] : mainS;
        if (!dry && (p->tun.dbg_streams & 8) && sideS != mainS) {   // (diagnostic: the content chain starts behind the dense-stack kernel and the speaker's dense weight gradients)
            hipEventRecord(p->ev_dense, sideS);
            hipStreamWaitEvent(mainS, p->ev_dense, 0);
        }
        if (do_enc) RUN(content_branch());
        if (!dry && (p->tun.dbg_streams & 4) && sideS != mainS) {   // (diagnostic: the speaker's conv chain starts behind the content chain)
            hipEventRecord(p->ev_join, mainS);
            hipStreamWaitEvent(sideS, p->ev_join, 0);
        }
        c.s = sideS;
        c.wstream = (overlap && sideS != mainS) ? p->wstream[1] : sideS;
        // pooled -> [B,C,Tn] ; dy2 of the last block masked by its ReLU output
        const int Tn = e.T[e.n];
        dyA = c.fresh((long)B * C * Tn);
        if (!dry) {
            if (bh) RUN(avc_launch_timepool_bwd_pairs(dhA, ws + e.a2[e.n - 1], B, Cc, Tn, gA, dyA, SL, s));
            else RUN(avc_launch_timepool_bwd(dhA, ws + e.a2[e.n - 1], B, Cc, Tn, gA, dyA, SL, s));
            avc_prof_mark(2, s);
        }
        for (int l = e.n - 1; l >= 0; --l) {
            const int Ti = e.T[l], T2 = e.T[l + 1], sub = e.c.subsample[l];
            const LayerP& L1 = p->layers[e.c1[l]];
            const LayerP& L2 = p->layers[e.c2[l]];
            // dyA = G_{l+1} * (a2 > 0)
            dyB = c.fresh((long)B * C * Ti);
            if (!dry) {
                ConvArgs a = mk_dgrad(SL, L2, ws, dyA, (long)C * T2, T2, 1, 1, B, T2, Ti, nullptr, (long)C * Ti, Ti, 1);
                a.g[0].out2 = dyB;
                a.g[0].mask = ws + e.a1[l];
                RUN(avc_launch_conv(a, s, 0, p->tun));
            }
            RUN(wgrad_layer(c, L2, ws + e.a1[l], (long)C * Ti, Ti, 1, dyA, (long)C * T2, T2, 1, 1, B, Ti, T2));
            dyA = c.fresh((long)B * C * Ti);  // (the wgrad of conv2 above still reads the previous dyA)
            if (!dry) {
                ConvArgs a = mk_dgrad(SL, L1, ws, dyB, (long)C * Ti, Ti, 1, 1, B, Ti, Ti, gC, (long)C * Ti, Ti, 1);
                set_res(a, gA, sub > 1 ? AVC_RES_POOLT : AVC_RES_IDENTITY, (long)C * T2, T2, 1, T2);
                a.g[0].out2 = dyA;  // next: dy2 of block l-1, or d(in_conv out) for l == 0
                a.g[0].mask = (l > 0) ? ws + e.a2[l - 1] : ws + e.h0;
                RUN(avc_launch_conv(a, s, 0, p->tun));
            }
            RUN(wgrad_layer(c, L1, ws + e.out[l], (long)C * Ti, Ti, 1, dyB, (long)C * Ti, Ti, 1, 1, B, Ti, Ti));
            rot();
        }
        RUN(enc_back_front(c, e, xc, scb, scc, sct, dyA));
        if (!dry) avc_prof_mark(4, s);
        RUN(flush_wgrads(c));
        // the speaker encoder's gradients (head of the flat buffer) are final once its wgrad stream drains: a data-parallel caller
        // reduces them under the content encoder's longer branch (avc_plan_stream_wait_grads(AVC_GRADS_SPEAKER))
        if (!dry && p->side_state == 1) hipEventRecord(p->ev_spk_grads, c.wstream);
        c.s = mainS;
        c.wstream = overlap ? p->wstream[0] : mainS;
    }
    if (!dry) join_side(p, mainS, sideS);
    if (overlap) {
        for (int i = 0; i < 2; ++i) {
            hipEventRecord(p->wjoin[i], p->wstream[i]);
            hipStreamWaitEvent(mainS, p->wjoin[i], 0);
        }
    }
    if (!dry && p->side_state == 1) hipEventRecord(p->ev_all_grads, s);
    if (!dry) avc_prof_mark(6, s);
    if (slab_need) {
        slab_need[0] = c.slab_used;
        slab_need[1] = c.dy_used;
        slab_need[2] = c.nev;
    }
    return 0;
}

extern "C" int avc_backward(const avc_plan* p, const float* params, const float* x, long sxb, long sxc, int sxt,
                            const float* x_cond, long scb, long scc, int sct, const float* eps, const float* d_dec,
                            const float* d_muls_up, const float* d_emb_up, float lambda_kl, float* grads, float* ws,
                            void* stream) {
    if (!p || !params || !x || !ws || !grads) return fail(-1, "avc_backward: null argument");
    if ((p->flags & AVC_PLAN_PARTS) && (p->flags & AVC_PLAN_INFERENCE))
        return fail(-8, "avc_backward: a part plan needs AVC_PLAN_PART_GRADS for its backward (no gradient buffers)");
    if (p->flags & AVC_PLAN_INFERENCE) return fail(-8, "avc_backward: the plan was created with AVC_PLAN_INFERENCE (no gradient buffers)");
    if (p->flags & AVC_PLAN_DECODER_ONLY) return fail(-8, "avc_backward: decoder part plans run through avc_decoder_backward");
    if ((p->flags & AVC_PLAN_CONTENT_ONLY) && (d_dec || d_emb_up))
        return fail(-1, "avc_backward: a content part plan takes d_muls_up only (d_dec and d_emb_up must be NULL)");
    if ((p->flags & AVC_PLAN_SPEAKER_ONLY) && (d_dec || d_muls_up || !d_emb_up))
        return fail(-1, "avc_backward: a speaker part plan takes d_emb_up only (d_dec and d_muls_up must be NULL)");
    const bool one_input = !x_cond;   // AE.forward: both encoders read x (a separate x_cond is another input, whatever memory it shares)
    if (!x_cond) {
        x_cond = x; scb = sxb; scc = sxc; sct = sxt;
    }
    const int rc = avc_backward_impl(p, params, x, sxb, sxc, sxt, x_cond, scb, scc, sct, eps, d_dec, d_muls_up, d_emb_up, lambda_kl,
                                     grads, ws, (hipStream_t)stream, false, nullptr);
    if (rc) return rc;
    // d(x) of a single input: the speaker encoder's term onto the content encoder's, behind the join of the two branches (fixed order)
    if (one_input && (p->flags & AVC_PLAN_INPUT_GRADS) && has_spk(p->flags) && has_enc(p->flags) && p->spk.T[0] == p->enc.T[0])
        RUN(avc_launch_add(ws + p->enc.dx, ws + p->spk.dx, (long)p->B * p->M * p->T, (hipStream_t)stream));
    return 0;
}

// autograd of Decoder.forward (model.py:347-371) on a decoder part plan with AVC_PLAN_PART_GRADS: the decoder's parameter gradients,
// ws["d_z"] and ws["d_emb"] (row-major) from d(dec); z / emb / params as handed to the avc_decoder_forward this pass follows
extern "C" int avc_decoder_backward(const avc_plan* p, const float* params, const float* z, long szb, long szc, int szt, const float* emb,
                                    long seb, long sec, const float* d_dec, float* grads, float* ws, void* stream) {
    if (!p || !params || !z || !emb || !ws || !grads) return fail(-1, "avc_decoder_backward: null argument");
    if (!(p->flags & AVC_PLAN_DECODER_ONLY)) return fail(-8, "avc_decoder_backward: the plan was not created with AVC_PLAN_DECODER_ONLY");
    if (p->flags & AVC_PLAN_INFERENCE) return fail(-8, "avc_decoder_backward: the plan was created without AVC_PLAN_PART_GRADS (no gradient buffers)");
    const DecIn din = {z, szb, szc, szt, emb, seb, sec};
    return avc_backward_impl(p, params, nullptr, 0, 0, 0, nullptr, 0, 0, 0, nullptr, d_dec, nullptr, nullptr, 0.f, grads, ws, (hipStream_t)stream,
                             false, nullptr, &din);
}


// --------------------------------------------------------------------------
// ragged inference: utterances of different lengths in ONE launch set
// --------------------------------------------------------------------------
static long rag_put(avc_plan* p, const std::vector<int>& v) {   // a table into the host image, 16-byte aligned
    long o = (long)p->rag_host.size();
    p->rag_host.insert(p->rag_host.end(), v.begin(), v.end());
    while (p->rag_host.size() % 4) p->rag_host.push_back(0);
    return o;
}
static void rag_level(avc_plan* p, avc_plan::RagLevel& L, const std::vector<int>& T) {
    const int B = (int)T.size();
    L.T = T;
    L.off.assign(B + 1, 0);
    for (int b = 0; b < B; ++b) L.off[b + 1] = L.off[b] + T[b];
    std::vector<int> tiles;
    for (int b = 0; b < B; ++b)
        for (int t0 = 0; t0 < T[b]; t0 += 64) {
            tiles.push_back(b);
            tiles.push_back(t0);
        }
    L.ntiles = (int)tiles.size() / 2;
    L.dT = rag_put(p, L.T);
    L.doff = rag_put(p, L.off);
    L.dtile = rag_put(p, tiles);
}

// Workspace of the ragged plans with a backward pass (AVC_PLAN_INPUT_GRADS).  The order of the allocations is the workspace layout.
// one branch, one stream, no weight gradient: two ping-pong pairs of gradient rows suffice
static void rag_alloc_grad_rows(avc_plan* p, long floats) {
    p->gA2 = p->alloc(floats);   // G_l: d(loss)/d(out_l), the residual path's gradient
    p->gC2 = p->alloc(floats);
    p->gA = p->alloc(floats);    // the gradients entering conv2 / conv1 of a block: masked (speaker), or what an InstanceNorm backward leaves
    p->gB = p->alloc(floats);
}
// row statistics of every InstanceNorm of an encoder / the decoder: mean[n * C] | rstd[n * C], row b * C + c
template <class Net>
static void rag_alloc_stats(avc_plan* p, Net& net, long n, long C) {
    net.st0 = p->alloc(2 * n * C);
    for (int l = 0; l < net.n; ++l) {
        net.st1[l] = p->alloc(2 * n * C);
        net.st2[l] = p->alloc(2 * n * C);
    }
}
static void rag_alloc_enc_input_grads(avc_plan* p, EncNet& e, long sumT) {
    e.dcat = p->alloc((long)e.CC * sumT);
    e.dx = p->alloc((long)e.c.c_in * sumT);
}
// named["<prefix>_<name>_<l>"] for every level l of every listed per-level buffer
static void rag_name_levels(avc_plan* p, const std::string& prefix, int n, std::initializer_list<std::pair<const char*, const long*>> bufs) {
    for (int l = 0; l < n; ++l)
        for (const auto& b : bufs) p->named[prefix + "_" + b.first + "_" + std::to_string(l)] = b.second[l];
}

static int rag_plan_create(const avc_model_cfg* cfg, int B, const int* T, const int* T_cond, int flags, int N, const int* src_of,
                           const avc_tuning* tuning, avc_plan** out);

extern "C" int avc_plan_create_ragged(const avc_model_cfg* cfg, int B, const int* T, const int* T_cond, const avc_tuning* tuning, avc_plan** out) {
    return avc_plan_create_ragged_ex(cfg, B, T, T_cond, 0, tuning, out);
}

// flags: 0 = B (source, target) pairs through all three networks; AVC_PLAN_SPEAKER_ONLY = the speaker encoder over T_cond alone;
// AVC_PLAN_EMB_INPUT = content encoder + decoder over T, the embeddings come from the caller (avc_forward_ragged_emb).  A network that
// does not run keeps its entries of the flat parameter buffer, and gets no weight image, no level table and no buffer.
extern "C" int avc_plan_create_ragged_ex(const avc_model_cfg* cfg, int B, const int* T, const int* T_cond, int flags, const avc_tuning* tuning,
                                         avc_plan** out) {
    if (flags & ~(AVC_PLAN_SPEAKER_ONLY | AVC_PLAN_EMB_INPUT | AVC_PLAN_INPUT_GRADS))
        return fail(-1, "avc_plan_create_ragged_ex: unknown flag (ragged plans take AVC_PLAN_SPEAKER_ONLY [| AVC_PLAN_INPUT_GRADS] or AVC_PLAN_EMB_INPUT)");
    if ((flags & AVC_PLAN_SPEAKER_ONLY) && (flags & AVC_PLAN_EMB_INPUT))
        return fail(-1, "avc_plan_create_ragged_ex: AVC_PLAN_SPEAKER_ONLY and AVC_PLAN_EMB_INPUT exclude each other");
    if ((flags & AVC_PLAN_INPUT_GRADS) && !(flags & AVC_PLAN_SPEAKER_ONLY))
        return fail(-1, "avc_plan_create_ragged_ex: unknown flag for this ragged plan: AVC_PLAN_INPUT_GRADS is supported on ragged speaker plans only, pass AVC_PLAN_SPEAKER_ONLY | "
                        "AVC_PLAN_INPUT_GRADS (the ragged content encoder and decoder have no backward pass; use uniform plans for their gradients)");
    return rag_plan_create(cfg, B, T, T_cond, flags, 0, nullptr, tuning, out);
}

// S sources, N outputs, output j decoded from source src_of[j] with row j of the caller's embeddings.  flags: 0 = content encoder over
// the sources + decoder over the outputs; AVC_PLAN_CONTENT_ONLY = the content encoder alone (N = 0); AVC_PLAN_DECODER_ONLY = the decoder
// alone, T are the latent lengths.  The speaker encoder never runs.
extern "C" int avc_plan_create_ragged_fanout(const avc_model_cfg* cfg, int S, const int* T, int N, const int* src_of, int flags,
                                             const avc_tuning* tuning, avc_plan** out) {
    if (flags & ~(AVC_PLAN_CONTENT_ONLY | AVC_PLAN_DECODER_ONLY))
        return fail(-1, "avc_plan_create_ragged_fanout: unknown flag (fan-out plans take 0, AVC_PLAN_CONTENT_ONLY or AVC_PLAN_DECODER_ONLY)");
    if ((flags & AVC_PLAN_CONTENT_ONLY) && (flags & AVC_PLAN_DECODER_ONLY))
        return fail(-1, "avc_plan_create_ragged_fanout: AVC_PLAN_CONTENT_ONLY and AVC_PLAN_DECODER_ONLY exclude each other");
    if (!cfg || !out || !T || S < 1) return fail(-1, "avc_plan_create_ragged_fanout: bad arguments (S >= 1 sources of T[s] frames)");
    if (flags & AVC_PLAN_CONTENT_ONLY) {
        if (N != 0 || src_of) return fail(-1, "avc_plan_create_ragged_fanout: a content-only plan has no outputs: N must be 0 and src_of NULL");
    } else {
        if (N < 1 || !src_of) return fail(-1, "avc_plan_create_ragged_fanout: N >= 1 outputs and their sources src_of[0..N) are needed");
        for (int j = 0; j < N; ++j)
            if (src_of[j] < 0 || src_of[j] >= S) return fail(-1, "avc_plan_create_ragged_fanout: src_of out of range (every entry must be a source index in [0, S))");
    }
    const int kind = (flags & AVC_PLAN_CONTENT_ONLY) ? AVC_PLAN_CONTENT_ONLY : (AVC_PLAN_EMB_INPUT | flags);
    return rag_plan_create(cfg, S, T, nullptr, AVC_PLAN_FANOUT | kind, N, src_of, tuning, out);
}

// The content encoder alone over S sources WITH a backward pass with respect to its input (avc_content_backward_ragged): the content-only
// fan-out plan plus the input-gradient weight images, the saved InstanceNorm statistics and the gradient rows.
extern "C" int avc_plan_create_ragged_content_grads(const avc_model_cfg* cfg, int S, const int* T, const avc_tuning* tuning, avc_plan** out) {
    if (!cfg || !out || !T || S < 1) return fail(-1, "avc_plan_create_ragged_content_grads: bad arguments (S >= 1 sources of T[s] frames)");
    return rag_plan_create(cfg, S, T, nullptr, AVC_PLAN_FANOUT | AVC_PLAN_CONTENT_ONLY | AVC_PLAN_INPUT_GRADS, 0, nullptr, tuning, out);
}

// The decoder alone over N latents WITH a backward pass with respect to its two inputs (avc_decoder_backward_ragged): output j from latent j
// (the identity map: no AVC_PLAN_FANOUT), the forward launches of the decoder-only fan-out plan over the same lengths, plus the
// input-gradient weight images, the saved InstanceNorm statistics, d(cond), the gradient rows, d(z) and d(emb).
extern "C" int avc_plan_create_ragged_decoder_grads(const avc_model_cfg* cfg, int N, const int* Tz, const avc_tuning* tuning, avc_plan** out) {
    if (!cfg || !out || !Tz || N < 1) return fail(-1, "avc_plan_create_ragged_decoder_grads: bad arguments (N >= 1 latents of Tz[j] frames)");
    return rag_plan_create(cfg, N, Tz, nullptr, AVC_PLAN_EMB_INPUT | AVC_PLAN_DECODER_ONLY | AVC_PLAN_INPUT_GRADS, 0, nullptr, tuning, out);
}

// The speaker encoder alone over B utterances WITH a backward pass that also computes its PARAMETER gradients (avc_backward_ragged_params):
// the flagged speaker plan of avc_plan_create_ragged_ex plus the weight gradient's chunk tables and split-K slots and one d(pre-activation)
// row set per dense layer.
extern "C" int avc_plan_create_ragged_speaker_grads(const avc_model_cfg* cfg, int B, const int* T_cond, const avc_tuning* tuning, avc_plan** out) {
    if (!cfg || !out || !T_cond || B < 1) return fail(-1, "avc_plan_create_ragged_speaker_grads: bad arguments (B >= 1 utterances of T_cond[b] frames)");
    return rag_plan_create(cfg, B, nullptr, T_cond, AVC_PLAN_SPEAKER_ONLY | AVC_PLAN_INPUT_GRADS | AVC_PLAN_PART_GRADS, 0, nullptr, tuning, out);
}

// The content encoder alone over S sources WITH a backward pass that also computes its PARAMETER gradients
// (avc_content_backward_ragged_params): the plan of avc_plan_create_ragged_content_grads plus the weight gradient's chunk tables on every
// level, one more set of gradient rows and the split-K slots.
extern "C" int avc_plan_create_ragged_content_param_grads(const avc_model_cfg* cfg, int S, const int* T, const avc_tuning* tuning, avc_plan** out) {
    if (!cfg || !out || !T || S < 1) return fail(-1, "avc_plan_create_ragged_content_param_grads: bad arguments (S >= 1 sources of T[s] frames)");
    return rag_plan_create(cfg, S, T, nullptr, AVC_PLAN_FANOUT | AVC_PLAN_CONTENT_ONLY | AVC_PLAN_INPUT_GRADS | AVC_PLAN_PART_GRADS, 0, nullptr, tuning, out);
}

// ... and the decoder alone over N latents (avc_decoder_backward_ragged_params): the plan of avc_plan_create_ragged_decoder_grads plus the same.
extern "C" int avc_plan_create_ragged_decoder_param_grads(const avc_model_cfg* cfg, int N, const int* Tz, const avc_tuning* tuning, avc_plan** out) {
    if (!cfg || !out || !Tz || N < 1) return fail(-1, "avc_plan_create_ragged_decoder_param_grads: bad arguments (N >= 1 latents of Tz[j] frames)");
    return rag_plan_create(cfg, N, Tz, nullptr, AVC_PLAN_EMB_INPUT | AVC_PLAN_DECODER_ONLY | AVC_PLAN_INPUT_GRADS | AVC_PLAN_PART_GRADS, 0, nullptr, tuning, out);
}

// the K-chunks of a level's weight gradient: 32 frames of one sample each, samples in order
static void rag_chunks(avc_plan* p, avc_plan::RagLevel& L) {
    std::vector<int> ch;
    for (int b = 0; b < (int)L.T.size(); ++b)
        for (int t0 = 0; t0 < L.T[b]; t0 += 32) {
            ch.push_back(b);
            ch.push_back(t0);
        }
    L.nchunks = (int)ch.size() / 2;
    L.dchunk = rag_put(p, ch);
}
// split and slots of layer L's ragged weight gradient over the chunks of the level its output lives on
// (a stacked layer -- the content encoder's two heads, the decoder's 2n affine Linears -- is nsrc tensors of `rows` output channels, each a
// job of its own; every other layer has nsrc = 1 and rows = Cout)
static void rag_wgrad_slots(avc_plan* p, LayerP& L, int nchunks) {
    L.rwg_nsplit = avc_rwg_nsplit(L.Cin, L.rows, nchunks);
    if (L.rwg_nsplit > 1) L.rwg_slab = p->alloc((long)L.nsrc * L.rwg_nsplit * avc_rwg_slot_floats(L.Cin, L.rows, L.KS));
}
static void rag_wgrad_slots(avc_plan* p, LayerP& L, const avc_plan::RagLevel& yl) { rag_wgrad_slots(p, L, yl.nchunks); }

// flags: what avc_plan_flags reports, minus INFERENCE | RAGGED.  With AVC_PLAN_FANOUT the decoder runs over N samples mapped onto the B
// sources by src_of; without it over the B sources themselves.
static int rag_plan_create(const avc_model_cfg* cfg, int B, const int* T, const int* T_cond, int flags, int N, const int* src_of,
                           const avc_tuning* tuning, avc_plan** out) {
    const bool ig = (flags & AVC_PLAN_INPUT_GRADS) != 0;
    const bool fan = (flags & AVC_PLAN_FANOUT) != 0;
    const bool do_spk = rag_has_spk(flags), do_enc = has_enc(flags), do_dec = has_dec(flags);
    const int Nd = do_dec ? (fan ? N : B) : 0;   // the decoder's sample count
    if (!do_enc && !do_dec) T = T_cond;   // (speaker-only: T is ignored; the shared length checks below then read T_cond twice)
    if (!cfg || !out || !T || B < 1) return fail(-1, "avc_plan_create_ragged: bad arguments");
    if (tuning && tuning->struct_size != (int)sizeof(avc_tuning)) return fail(-1, "avc_plan_create_ragged: avc_tuning of another library version (use avc_tuning_init)");
    if (!T_cond || !do_spk) T_cond = T;
    if (int rc = check_model_cfg(*cfg, "avc_plan_create_ragged")) return rc;
    const avc_decoder_cfg& dc = cfg->dec;

    avc_plan* p = new avc_plan();
    p->cfg = *cfg;
    p->flags = AVC_PLAN_INFERENCE | AVC_PLAN_RAGGED | flags;
    p->tun = tuning ? *tuning : avc_default_tuning();
    p->tun.ck16_wgs = -1;   // default chunk depths: the ragged launcher has the straight-line instances for those
    p->tun.ck32_wgs = -1;
    p->tun.conv_x3 = 0;
    p->B = B;
    p->Nd = Nd;
    p->M = cfg->enc.c_in;
    p->T = p->Tc = 0;
    for (int b = 0; b < B; ++b) {
        if (T[b] < 1 || T_cond[b] < 1) { delete p; return fail(-1, "avc_plan_create_ragged: lengths must be positive"); }
        p->T = T[b] > p->T ? T[b] : p->T;
        p->Tc = T_cond[b] > p->Tc ? T_cond[b] : p->Tc;
    }
    build_enc_params(p, p->spk, cfg->spk, true);
    p->enc_param_off = p->param_floats;
    build_enc_params(p, p->enc, cfg->enc, false);
    build_dec_params(p);
    DecNet& d = p->dec;

    // ---- per-sample time schedules; the reference's reflect-pad rule per utterance
    auto sched = [&](EncNet& e, const int* T0, std::vector<avc_plan::RagLevel>& lv) -> int {
        std::vector<int> cur(T0, T0 + B);
        lv.resize(e.n + 1);
        for (int b = 0; b < B; ++b)
            if (e.c.bank_size / 2 >= cur[b]) return -1;
        for (int l = 0; l <= e.n; ++l) {
            rag_level(p, lv[l], cur);
            if (l == e.n) break;
            for (int b = 0; b < B; ++b) {
                if (e.c.kernel_size / 2 >= cur[b]) return -1;
                cur[b] = avc_cdiv(cur[b], e.c.subsample[l]);
            }
        }
        return 0;
    };
    bool bad = (do_spk && sched(p->spk, T_cond, p->rl_spk) != 0) || (do_enc && sched(p->enc, T, p->rl_enc) != 0);
    if (!bad && do_dec) {
        std::vector<int> cur = do_enc ? p->rl_enc[p->enc.n].T : std::vector<int>(T, T + B);   // (decoder-only: T are the latent lengths)
        if (fan) {   // the sources' latent level, and every output's source in it
            if (do_enc) p->rl_z = p->rl_enc[p->enc.n];   // (the tables the heads write by: no second copy)
            else rag_level(p, p->rl_z, cur);
            avc_plan::RagLevel& m = p->rl_map;
            m.T.resize(Nd);
            m.off.resize(Nd);
            for (int j = 0; j < Nd; ++j) {
                m.T[j] = p->rl_z.T[src_of[j]];
                m.off[j] = p->rl_z.off[src_of[j]];
            }
            m.dT = rag_put(p, m.T);
            m.doff = rag_put(p, m.off);
            cur = m.T;
        }
        p->rl_dec.resize(d.n + 1);
        for (int l = 0; l <= d.n && !bad; ++l) {
            rag_level(p, p->rl_dec[l], cur);
            if (l == d.n) break;
            for (int b = 0; b < Nd; ++b) {
                if (dc.kernel_size / 2 >= cur[b]) bad = true;
                cur[b] *= dc.upsample[l];
            }
        }
    }
    if (bad) {
        delete p;
        return fail(-6, "Padding size should be less than the corresponding input dimension");
    }
    p->Tb = 0;
    p->Tout = 0;

    // ---- packed weights (forward images only); tile heuristics see the launch's column-tile count as its batch
    for (EncNet* e : {&p->spk, &p->enc}) {
        if (!(e == &p->spk ? do_spk : do_enc)) continue;
        const std::vector<avc_plan::RagLevel>& lv = (e == &p->spk) ? p->rl_spk : p->rl_enc;
        // (AVC_PLAN_INPUT_GRADS -- a speaker plan, or the content plan of avc_plan_create_ragged_content_grads -- adds the input-gradient
        // images: transposed, tap-flipped)
        for (int id : e->bank) finish_layer(p, p->layers[id], ig, 0, lv[0].ntiles, 64, 64, e->nb);
        finish_layer(p, p->layers[e->in_conv], ig, e->CC - e->c.c_in, lv[0].ntiles, 64, 64);
        if (ig) {   // the in_conv's input gradient for its last M input rows (x itself, model.py:90): w[0] rows [nb c_bank, CC)
            LayerP L = p->layers[e->in_conv];
            L.src_off = (long)e->nb * e->c.c_bank;
            L.wpf = L.wrs_f = L.wrs_d = L.wplain = L.bpk = -1;
            L.dgM = e->c.c_in;
            L.Mp_d = avc_cdiv(L.dgM, 128) * 128;
            L.wpd = p->alloc((long)L.nchunk_d * L.KS * L.CKd * L.Mp_d);
            p->layers.push_back(L);
            e->in_pass = (int)p->layers.size() - 1;
        }
        for (int l = 0; l < e->n; ++l) {
            finish_layer(p, p->layers[e->c1[l]], ig, 0, lv[l].ntiles, 64, 64);
            finish_layer(p, p->layers[e->c2[l]], ig, 0, lv[l + 1].ntiles, 64, 64);
        }
    }
    if (do_spk) {
        for (int l = 0; l < p->spk.nd; ++l) {
            finish_layer(p, p->layers[p->spk.dn1[l]], ig, 0, 1, B, B, 1, false);
            finish_layer(p, p->layers[p->spk.dn2[l]], ig, 0, 1, B, B, 1, false);
        }
        finish_layer(p, p->layers[p->spk.outl], ig, 0, 1, B, B, 1, false);
    }
    // every layer gets the tile count of the level it runs over: the sources' for the encoder, its heads and the decoder's in_conv, the
    // outputs' for the decoder's blocks and out_conv (the same numbers wherever sources and outputs are the same samples)
    const avc_plan::RagLevel* lz = do_dec ? (fan ? &p->rl_z : &p->rl_dec[0]) : (do_enc ? &p->rl_enc[p->enc.n] : nullptr);
    if (do_enc) finish_layer(p, p->layers[p->enc.heads], ig, 0, p->rl_enc[p->enc.n].ntiles, 64, 64);
    if (do_dec) {
        // (ig: the plan of avc_plan_create_ragged_decoder_grads adds the input-gradient images)
        finish_layer(p, p->layers[d.in_conv], ig, 0, lz->ntiles, 64, 64);
        for (int l = 0; l < d.n; ++l) {
            finish_layer(p, p->layers[d.c1[l]], ig, 0, p->rl_dec[l].ntiles, 64, 64);
            finish_layer(p, p->layers[d.c2[l]], ig, 0, p->rl_dec[l].ntiles, 64, 64);
        }
        finish_layer(p, p->layers[d.affine], ig, 0, 1, Nd, Nd);
        finish_layer(p, p->layers[d.out_conv], ig, 0, p->rl_dec[d.n].ntiles, 64, 64);
    }

    // ---- packed activation buffers: [channels][T_b] blocks back to back
    const long Bl = B;
    auto alloc_enc = [&](EncNet& e, const std::vector<avc_plan::RagLevel>& lv, bool spk) {
        const long C = e.c.c_h;
        e.cat = p->alloc((long)e.CC * lv[0].off[B]);
        e.h0 = p->alloc(C * lv[0].off[B]);
        e.out[0] = spk ? e.h0 : p->alloc(C * lv[0].off[B]);
        for (int l = 0; l < e.n; ++l) {
            e.a1[l] = p->alloc(C * lv[l].off[B]);
            e.out[l + 1] = p->alloc(C * lv[l + 1].off[B]);
            if (spk) {
                e.a2[l] = p->alloc(C * lv[l + 1].off[B]);
                e.y1[l] = e.y2[l] = -1;
            } else {
                e.a2[l] = -1;
                e.y1[l] = p->alloc(C * lv[l].off[B]);
                e.y2[l] = p->alloc(C * lv[l + 1].off[B]);
            }
        }
        if (spk) {
            e.pooled = p->alloc(C * Bl);
            e.hd[0] = e.pooled;
            for (int l = 0; l < e.nd; ++l) {
                e.d1[l] = p->alloc(C * Bl);
                e.d2[l] = p->alloc(C * Bl);
                e.hd[l + 1] = p->alloc(C * Bl);
            }
        }
    };
    const long Cz = dc.c_in, Cd = dc.c_h;
    if (do_spk) {
        alloc_enc(p->spk, p->rl_spk, true);
        p->emb = p->alloc(Bl * dc.c_cond);
        p->named["emb"] = p->emb;
    }
    if (ig && do_spk) {   // avc_backward_ragged: d(cat), d(x_cond), the gradient rows, the dense stack's temporaries
        EncNet& e = p->spk;
        const long C = e.c.c_h, sumT = p->rl_spk[0].off[B];
        rag_alloc_enc_input_grads(p, e, sumT);
        rag_alloc_grad_rows(p, C * sumT);
        p->demb = p->alloc(Bl * dc.c_cond);
        p->dhA = p->alloc(C * Bl);
        p->dz = p->alloc(C * Bl);       // the dense stack's d(pre-activation) rows: written by its backward kernel, read by nobody (no weight gradient)
        p->named["d_x_cond"] = e.dx;
        // the saved activations the backward pass masks by (tests read the ReLU branch the engine took from them)
        p->named["spk_cat"] = e.cat;
        p->named["spk_h0"] = e.h0;
        rag_name_levels(p, "spk", e.n, {{"a1", e.a1}, {"a2", e.a2}});
        rag_name_levels(p, "spk", e.nd, {{"d1", e.d1}, {"d2", e.d2}});
        if (flags & AVC_PLAN_PART_GRADS) {   // avc_backward_ragged_params: chunk tables, one dz row set per dense layer, the split-K slots
            for (avc_plan::RagLevel& l : p->rl_spk) rag_chunks(p, l);
            rag_level(p, p->rl_dense, std::vector<int>(1, B));
            rag_chunks(p, p->rl_dense);
            for (int l = 0; l < 2 * e.nd; ++l) p->rag_dz.push_back(p->alloc(C * Bl));
            for (int id : e.bank) rag_wgrad_slots(p, p->layers[id], p->rl_spk[0]);
            rag_wgrad_slots(p, p->layers[e.in_conv], p->rl_spk[0]);
            for (int l = 0; l < e.n; ++l) {
                rag_wgrad_slots(p, p->layers[e.c1[l]], p->rl_spk[l]);
                rag_wgrad_slots(p, p->layers[e.c2[l]], p->rl_spk[l + 1]);
            }
            for (int l = 0; l < e.nd; ++l) {
                rag_wgrad_slots(p, p->layers[e.dn1[l]], p->rl_dense);
                rag_wgrad_slots(p, p->layers[e.dn2[l]], p->rl_dense);
            }
            rag_wgrad_slots(p, p->layers[e.outl], p->rl_dense);
        }
    }
    if (do_enc) {
        alloc_enc(p->enc, p->rl_enc, false);
        p->muls = p->alloc(2 * Cz * lz->off[B]);
        p->named["muls"] = p->muls;
    }
    if (ig && do_enc) {   // avc_content_backward_ragged: row statistics of every InstanceNorm, d(cat), d(x), two ping-pong pairs of gradient rows
        EncNet& e = p->enc;
        const long C = e.c.c_h, sumT = p->rl_enc[0].off[B];
        rag_alloc_stats(p, e, Bl, C);
        rag_alloc_enc_input_grads(p, e, sumT);
        rag_alloc_grad_rows(p, C * sumT);
        p->named["d_x"] = e.dx;
        // what the backward pass masks by (tests read the ReLU branch the engine took: cat > 0, saved y > saved row mean)
        p->named["enc_cat"] = e.cat;
        p->named["enc_y0"] = e.h0;
        p->named["enc_st0"] = e.st0;
        rag_name_levels(p, "enc", e.n, {{"y1", e.y1}, {"y2", e.y2}, {"st1", e.st1}, {"st2", e.st2}});
        if (flags & AVC_PLAN_PART_GRADS) {   // avc_content_backward_ragged_params: chunk tables, conv1's own dy rows, the split-K slots
            for (avc_plan::RagLevel& l : p->rl_enc) rag_chunks(p, l);
            p->rag_dy1 = p->alloc(C * sumT);
            for (int id : e.bank) rag_wgrad_slots(p, p->layers[id], p->rl_enc[0]);
            rag_wgrad_slots(p, p->layers[e.in_conv], p->rl_enc[0]);
            for (int l = 0; l < e.n; ++l) {
                rag_wgrad_slots(p, p->layers[e.c1[l]], p->rl_enc[l]);
                rag_wgrad_slots(p, p->layers[e.c2[l]], p->rl_enc[l + 1]);
            }
            rag_wgrad_slots(p, p->layers[e.heads], p->rl_enc[e.n]);
        }
    }
    if (do_dec) {   // the in_conv stage lives on the B sources' level, everything above on the Nd outputs' levels
        d.cond = p->alloc((long)Nd * 2 * d.n * 2 * Cd);
        d.y0 = p->alloc(Cd * lz->off[B]);
        d.out[0] = p->alloc(Cd * lz->off[B]);
        for (int l = 0; l < d.n; ++l) {
            d.y1[l] = p->alloc(Cd * p->rl_dec[l].off[Nd]);
            d.a1[l] = p->alloc(Cd * p->rl_dec[l].off[Nd]);
            d.y2[l] = p->alloc(Cd * p->rl_dec[l + 1].off[Nd]);
            d.out[l + 1] = p->alloc(Cd * p->rl_dec[l + 1].off[Nd]);
        }
        p->decb = p->alloc((long)p->M * p->rl_dec[d.n].off[Nd]);
        p->named["dec"] = p->decb;
        p->named["cond"] = d.cond;
    }
    if (ig && do_dec) {   // avc_decoder_backward_ragged: row statistics of every InstanceNorm, d(cond), two ping-pong pairs of gradient rows, d(z), d(emb)
        const long Nl = Nd, top = p->rl_dec[d.n].off[Nd];   // (the last level is the longest: upsample factors are 1 or 2)
        rag_alloc_stats(p, d, Nl, Cd);
        d.dcond = p->alloc(Nl * 2 * d.n * 2 * Cd);
        rag_alloc_grad_rows(p, Cd * top);
        p->dz = p->alloc(Cz * lz->off[B]);
        p->demb_rm = p->alloc(Nl * dc.c_cond);
        p->named["d_z"] = p->dz;
        p->named["d_emb"] = p->demb_rm;
        p->named["d_cond"] = d.dcond;
        // what the backward pass masks by (tests read the activation branch the engine took from the saved rows and statistics)
        p->named["dec_y0"] = d.y0;
        p->named["dec_st0"] = d.st0;
        rag_name_levels(p, "dec", d.n, {{"y1", d.y1}, {"a1", d.a1}, {"y2", d.y2}, {"st1", d.st1}, {"st2", d.st2}});
        if (flags & AVC_PLAN_PART_GRADS) {   // avc_decoder_backward_ragged_params: chunk tables, conv1's own dy rows, the split-K slots
            for (avc_plan::RagLevel& l : p->rl_dec) rag_chunks(p, l);
            p->rag_dy1 = p->alloc(Cd * top);
            rag_wgrad_slots(p, p->layers[d.in_conv], p->rl_dec[0]);
            for (int l = 0; l < d.n; ++l) {   // (conv2's dy lies as its own [C up][T_l] output rows: level l for both convs)
                rag_wgrad_slots(p, p->layers[d.c1[l]], p->rl_dec[l]);
                rag_wgrad_slots(p, p->layers[d.c2[l]], p->rl_dec[l]);
            }
            rag_wgrad_slots(p, p->layers[d.affine], avc_cdiv(Nd, 32));   // (strided jobs: the Nd samples are the frames)
            rag_wgrad_slots(p, p->layers[d.out_conv], p->rl_dec[d.n]);
        }
    }
    p->rag_tab = p->alloc((long)p->rag_host.size());
    plan_init_streams(p);
    *out = p;
    return 0;
}

extern "C" int avc_plan_ragged_out(const avc_plan* p, int* out_len, long* out_off) {
    if (!p || !(p->flags & AVC_PLAN_RAGGED) || !out_len || !out_off) return fail(-1, "avc_plan_ragged_out: not a ragged plan");
    if (p->flags & AVC_PLAN_SPEAKER_ONLY) return fail(-8, "avc_plan_ragged_out: a speaker-only ragged plan converts nothing (its result is ws[\"emb\"])");
    if (p->flags & AVC_PLAN_CONTENT_ONLY)
        return fail(-8, "avc_plan_ragged_out: a content-only ragged plan decodes nothing (its result is ws[\"muls\"]: avc_plan_ragged_latents)");
    const avc_plan::RagLevel& L = p->rl_dec[p->dec.n];
    for (int b = 0; b < p->Nd; ++b) {
        out_len[b] = L.T[b];
        out_off[b] = p->decb + (long)p->M * L.off[b];
    }
    return 0;
}

// where the content codes of every SOURCE lie: its latent length and the float offset of its [2 c_out][len] block (mu rows first)
extern "C" int avc_plan_ragged_latents(const avc_plan* p, int* len, long* off) {
    if (!p || !(p->flags & AVC_PLAN_RAGGED) || !len || !off) return fail(-1, "avc_plan_ragged_latents: not a ragged plan");
    if (p->flags & AVC_PLAN_SPEAKER_ONLY)
        return fail(-8, "avc_plan_ragged_latents: a speaker-only ragged plan has no content encoder (its result is ws[\"emb\"])");
    if (p->flags & AVC_PLAN_DECODER_ONLY)
        return fail(-8, "avc_plan_ragged_latents: a decoder-only ragged plan has no content encoder (its latents are the caller's: avc_decoder_forward_ragged)");
    const avc_plan::RagLevel& L = p->rl_enc[p->enc.n];
    for (int b = 0; b < p->B; ++b) {
        len[b] = L.T[b];
        off[b] = p->muls + (long)2 * p->cfg.enc.c_out * L.off[b];
    }
    return 0;
}

static void set_rag(ConvArgs& a, const int* tab, const avc_plan::RagLevel& src, int cx, const avc_plan::RagLevel& outl, const avc_plan::RagLevel& convl,
                    int cout) {
    // src: level of the source rows; convl: level whose lengths are the conv's output lengths (tiles run over it); outl: level
    // of the packed OUTPUT buffer (== convl unless the store pixel-shuffles)
    a.rag.tile = tab + convl.dtile;
    a.rag.ntiles = convl.ntiles;
    a.rag.Tsrc = tab + src.dT;
    a.rag.offsrc = tab + src.doff;
    a.rag.Tout = tab + convl.dT;
    a.rag.offout = tab + outl.doff;
    a.rag.cx = cx;
    a.rag.cout = cout;
    a.Tout = 64;    // geometry of a one-sample column tile
    a.Tsrc = 1 << 20;   // (per sample in the tables; the reflect-pad rule was checked per utterance at plan creation)
    a.B = 1;
    a.x.sb = 0;
    a.ob = 0;
}
static void set_rag_res(ConvArgs& a, const int* tab, const float* res, int mode, const avc_plan::RagLevel& rl, int cres) {
    a.g[0].res = res;
    a.res_mode = mode;
    a.rag.Tres = tab + rl.dT;
    a.rag.offres = tab + rl.doff;
    a.rag.cres = cres;
    a.rt = 1;
}

static int rag_in(int Bn, float slope, const int* tab, const float* y, float* out, const avc_plan::RagLevel& lv, int C, const float* cond, long csb,
                  int coff, const float* res, int res_mode, const avc_plan::RagLevel* rl, hipStream_t s, float* stats = nullptr) {
    RagINArgs a;
    memset(&a, 0, sizeof(a));
    a.y = y; a.out = out; a.T = tab + lv.dT; a.off = tab + lv.doff;
    a.cond = cond; a.cond_sb = csb; a.cond_off = coff;
    a.res = res; a.res_mode = res ? res_mode : 0;
    if (res) { a.Tres = tab + rl->dT; a.offres = tab + rl->doff; }
    a.B = Bn; a.C = C; a.slope = slope;   // (samples of level lv; the residual tables rl are indexed by the same sample)
    if (stats) { a.mean = stats; a.rstd = stats + (long)Bn * C; }   // (plans with a backward pass keep the row statistics)
    return avc_launch_rag_in_fwd(a, s);
}

static int rag_enc_front(const avc_plan* p, const EncNet& e, const std::vector<avc_plan::RagLevel>& lv, const int* tab, const float* params, float* ws,
                         const float* x, hipStream_t s) {
    // conv_bank (model.py:85-91) on the packed input [sum T][M] (frames as rows): channel stride 1, frame stride M
    const int M = e.c.c_in;
    const float SL = e.slope;
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.x.ptr = x; a.x.sc = 1; a.x.st = M; a.x.ps = 1;
    a.Cred = M; a.mode = 0; a.stride = 1; a.bf16 = p->compute;
    a.M = e.c.c_bank; a.Mp = avc_cdiv(e.c.c_bank, 128) * 128;
    a.ot = 1; a.ops = 1; a.act = 1; a.slope = SL;
    a.ngroups = e.nb;
    a.img = AVC_IMG_K4;
    for (int g = 0; g < e.nb; ++g) {
        const LayerP& L = p->layers[e.bank[g]];
        set_group(a.g[g], ws + L.wpf, p->par(params, L.b[0]), L.KS, L.CK, L.nchunk_f);
        a.g[g].out = ws + e.cat;
        a.g[g].out_c0 = g * e.c.c_bank;
    }
    set_rag(a, tab, lv[0], M, lv[0], lv[0], e.CC);
    RUN(avc_launch_conv(a, s, 0, p->tun));
    RUN(avc_launch_rag_copy_rows(x, 1, M, tab + lv[0].dT, tab + lv[0].doff, p->B, M, lv[0].off[p->B], ws + e.cat, e.CC, e.nb * e.c.c_bank, s));
    return 0;
}

// The ragged forward pass.  emb != NULL (AVC_PLAN_EMB_INPUT plans): the decoder's AdaIN affine GEMM reads the caller's embeddings in
// place (element strides seb, sec) and the speaker encoder does not run; otherwise it reads ws["emb"], the speaker encoder's result.
// z != NULL (decoder-only fan-out plans): the decoder's in_conv reads the caller's latent blocks of zc channels in place of ws["muls"].
static int rag_forward_impl(const avc_plan* p, const float* params, const float* x, const float* x_cond, const float* emb, long seb, long sec,
                            const float* z, int zc, float* ws, hipStream_t s) {
    const bool do_spk = rag_has_spk(p->flags), do_enc = has_enc(p->flags), do_dec = has_dec(p->flags);
    const int B = p->B;
    // tables -> workspace (a few KB; stream-ordered in front of everything that reads them)
    RUN((int)hipMemcpyAsync(ws + p->rag_tab, p->rag_host.data(), p->rag_host.size() * sizeof(int), hipMemcpyHostToDevice, s));
    const int* tab = (const int*)(ws + p->rag_tab);
    RUN(pack_all(p, params, ws, s));   // weights -> LDS-image order (one launch)
    // A conv on packed activations: source rows of the sample's own length (x.sc = -1), output block of `cout` channels.
    auto conv = [&](float slope, const LayerP& L, const float* src, const avc_plan::RagLevel& sl, int cx, float* dst, const avc_plan::RagLevel& convl,
                    const avc_plan::RagLevel& outl, int cout, int act, int ops) {
        ConvArgs a;
        memset(&a, 0, sizeof(a));
        a.x.ptr = src; a.x.sc = -1; a.x.st = 1; a.x.ps = 1;
        a.Cred = L.Cin; a.mode = 0; a.stride = L.stride; a.bf16 = L.bf16;
        a.M = L.Cout; a.Mp = L.Mp_f;
        a.ngroups = 1;
        set_group(a.g[0], ws + L.wpf, layer_bias(p, L, params, ws), L.KS, L.CK, L.nchunk_f);
        a.img = AVC_IMG_K4;
        a.ot = 1; a.ops = ops; a.act = act; a.slope = slope;
        a.g[0].out = dst;
        set_rag(a, tab, sl, cx, outl, convl, cout);
        return a;
    };
    const hipStream_t mainS = s;
    // two branches: the speaker encoder runs on the side stream beside the content encoder.  A plan with one of them has nothing to overlap
    // (and nothing to join): every kernel goes to the caller's stream
    const hipStream_t sideS = (do_spk && do_enc) ? fork_side(p, mainS) : mainS;
    if (do_spk) {   // ---------------- speaker encoder on the target utterances (model.py:265-277)
        const hipStream_t s = sideS;
        const EncNet& e = p->spk;
        const float SL = e.slope;
        const std::vector<avc_plan::RagLevel>& lv = p->rl_spk;
        const int C = e.c.c_h;
        RUN(rag_enc_front(p, e, lv, tab, params, ws, x_cond, s));
        {
            ConvArgs a = conv(SL, p->layers[e.in_conv], ws + e.cat, lv[0], e.CC, ws + e.h0, lv[0], lv[0], C, 1, 1);
            RUN(avc_launch_conv(a, s, 0, p->tun));
        }
        for (int l = 0; l < e.n; ++l) {
            ConvArgs a = conv(SL, p->layers[e.c1[l]], ws + e.out[l], lv[l], C, ws + e.a1[l], lv[l], lv[l], C, 1, 1);
            RUN(avc_launch_conv(a, s, 0, p->tun));
            ConvArgs b = conv(SL, p->layers[e.c2[l]], ws + e.a1[l], lv[l], C, ws + e.a2[l], lv[l + 1], lv[l + 1], C, 1, 1);
            b.g[0].out2 = ws + e.out[l + 1];
            set_rag_res(b, tab, ws + e.out[l], e.c.subsample[l] > 1 ? AVC_RES_AVGPOOL2 : AVC_RES_IDENTITY, lv[l], C);
            RUN(avc_launch_conv(b, s, 0, p->tun));
        }
        RUN(avc_launch_rag_timepool_fwd(ws + e.out[e.n], tab + lv[e.n].dT, tab + lv[e.n].doff, B, C, ws + e.pooled, s));
        DenseArgs da = dense_stack_args(p, e, params, ws, false);
        da.in = ws + e.hd[0];
        da.emb = ws + p->emb;
        for (int l = 0; l < e.nd; ++l) da.layer[2 * l + 1].out2 = ws + e.hd[l + 1];
        RUN(avc_launch_dense(da, 0, s));
    }
    if (do_enc) {   // ---------------- content encoder on the source utterances (model.py:301-323)
        const EncNet& e = p->enc;
        const float SL = e.slope;
        const std::vector<avc_plan::RagLevel>& lv = p->rl_enc;
        const int C = e.c.c_h;
        RUN(rag_enc_front(p, e, lv, tab, params, ws, x, s));
        const bool keep_stats = (p->flags & AVC_PLAN_INPUT_GRADS) != 0;   // (avc_plan_create_ragged_content_grads plans: the row statistics stay)
        auto st = [&](long off) -> float* { return keep_stats ? ws + off : nullptr; };
        {
            ConvArgs a = conv(SL, p->layers[e.in_conv], ws + e.cat, lv[0], e.CC, ws + e.h0, lv[0], lv[0], C, 0, 1);
            RUN(avc_launch_conv(a, s, 0, p->tun));
            RUN(rag_in(B, SL, tab, ws + e.h0, ws + e.out[0], lv[0], C, nullptr, 0, 0, nullptr, 0, nullptr, s, st(e.st0)));
        }
        for (int l = 0; l < e.n; ++l) {
            ConvArgs a = conv(SL, p->layers[e.c1[l]], ws + e.out[l], lv[l], C, ws + e.y1[l], lv[l], lv[l], C, 0, 1);
            RUN(avc_launch_conv(a, s, 0, p->tun));
            RUN(rag_in(B, SL, tab, ws + e.y1[l], ws + e.a1[l], lv[l], C, nullptr, 0, 0, nullptr, 0, nullptr, s, st(e.st1[l])));
            ConvArgs b = conv(SL, p->layers[e.c2[l]], ws + e.a1[l], lv[l], C, ws + e.y2[l], lv[l + 1], lv[l + 1], C, 0, 1);
            RUN(avc_launch_conv(b, s, 0, p->tun));
            RUN(rag_in(B, SL, tab, ws + e.y2[l], ws + e.out[l + 1], lv[l + 1], C, nullptr, 0, 0, ws + e.out[l],
                       e.c.subsample[l] > 1 ? AVC_RES_AVGPOOL2 : AVC_RES_IDENTITY, &lv[l], s, st(e.st2[l])));
        }
        ConvArgs h = conv(SL, p->layers[e.heads], ws + e.out[e.n], lv[e.n], C, ws + p->muls, lv[e.n], lv[e.n], 2 * e.c.c_out, 0, 1);
        RUN(avc_launch_conv(h, s, 0, p->tun));
    }
    join_side(p, mainS, sideS);
    if (do_dec) {   // ---------------- decoder(mu, emb) (model.py:347-371, :387-391: no noise)
        const DecNet& d = p->dec;
        const float SL = d.slope;
        const std::vector<avc_plan::RagLevel>& lv = p->rl_dec;
        const int C = d.c.c_h, Cz = d.c.c_in;
        const long csb = (long)2 * d.n * 2 * C;
        // Fan-out plans: the B sources' latent level lz carries the voice-independent in_conv stage ONCE per source; block 0 enters the
        // Nd outputs' levels through lm, which gives every output sample the length and the block offset of ITS source (the kernels
        // index every table by the tile's / row's sample).  Everywhere else sources and outputs are the same samples.
        const bool fan = (p->flags & AVC_PLAN_FANOUT) != 0;
        const avc_plan::RagLevel& lz = fan ? p->rl_z : lv[0];
        const avc_plan::RagLevel& lm = fan ? p->rl_map : lv[0];
        const int Nd = p->Nd;
        const float* es = emb ? emb : ws + p->emb;
        const long esb = emb ? seb : d.c.c_cond, esc = emb ? sec : 1;
        const bool keep_stats = (p->flags & AVC_PLAN_INPUT_GRADS) != 0;   // (avc_plan_create_ragged_decoder_grads plans: the row statistics stay)
        auto st = [&](long off) -> float* { return keep_stats ? ws + off : nullptr; };
        {   // all 2n AdaIN affine Linears as ONE GEMM on emb (uniform: one row per utterance; esb = 0: every utterance reads the same row)
            ConvArgs a = mk_fwd(p, SL, p->layers[d.affine], params, ws, es, 0, esc, (int)esb, 1, Nd, ws + d.cond, 0, 1, (int)csb, 0);
            RUN(avc_launch_conv(a, s, 0, p->tun));
        }
        {   // z = mu: the first Cz channels of every sample's (mu | log_sigma) block
            ConvArgs a = conv(SL, p->layers[d.in_conv], z ? z : ws + p->muls, lz, z ? zc : 2 * Cz, ws + d.y0, lz, lz, C, 0, 1);
            RUN(avc_launch_conv(a, s, 0, p->tun));
            RUN(rag_in(B, SL, tab, ws + d.y0, ws + d.out[0], lz, C, nullptr, 0, 0, nullptr, 0, nullptr, s, st(d.st0)));
        }
        for (int l = 0; l < d.n; ++l) {
            const int up = d.c.upsample[l];
            const avc_plan::RagLevel& lin = l == 0 ? lm : lv[l];   // where out[l] lies: block 0 reads the sources' blocks
            ConvArgs a = conv(SL, p->layers[d.c1[l]], ws + d.out[l], lin, C, ws + d.y1[l], lv[l], lv[l], C, 0, 1);
            RUN(avc_launch_conv(a, s, 0, p->tun));
            RUN(rag_in(Nd, SL, tab, ws + d.y1[l], ws + d.a1[l], lv[l], C, ws + d.cond, csb, (2 * l) * 2 * C, nullptr, 0, nullptr, s, st(d.st1[l])));
            // second conv: C * up channels, pixel-shuffled on store into the level-(l+1) buffer (model.py:359-361)
            ConvArgs b = conv(SL, p->layers[d.c2[l]], ws + d.a1[l], lv[l], C, ws + d.y2[l], lv[l], lv[l + 1], C, 0, up);
            RUN(avc_launch_conv(b, s, 0, p->tun));
            RUN(rag_in(Nd, SL, tab, ws + d.y2[l], ws + d.out[l + 1], lv[l + 1], C, ws + d.cond, csb, (2 * l + 1) * 2 * C, ws + d.out[l],
                       up > 1 ? AVC_RES_UP2 : AVC_RES_IDENTITY, &lin, s, st(d.st2[l])));
        }
        ConvArgs o = conv(SL, p->layers[d.out_conv], ws + d.out[d.n], lv[d.n], C, ws + p->decb, lv[d.n], lv[d.n], p->M, 0, 1);
        RUN(avc_launch_conv(o, s, 0, p->tun));
    }
    return 0;
}

extern "C" int avc_forward_ragged(const avc_plan* p, const float* params, const float* x, const float* x_cond, float* ws, void* stream) {
    if (!p || !params || !ws) return fail(-1, "avc_forward_ragged: null argument");
    if (!(p->flags & AVC_PLAN_RAGGED)) return fail(-8, "avc_forward_ragged: the plan was not created by avc_plan_create_ragged");
    if (p->flags & AVC_PLAN_DECODER_ONLY) return fail(-8, "avc_forward_ragged: decoder-only ragged plans run through avc_decoder_forward_ragged");
    if (p->flags & AVC_PLAN_EMB_INPUT) return fail(-8, "avc_forward_ragged: AVC_PLAN_EMB_INPUT plans run through avc_forward_ragged_emb");
    if (p->flags & AVC_PLAN_SPEAKER_ONLY) {
        if (!x_cond) return fail(-1, "avc_forward_ragged: a speaker-only plan reads x_cond (x is ignored), it must not be NULL");
        return rag_forward_impl(p, params, nullptr, x_cond, nullptr, 0, 0, nullptr, 0, ws, (hipStream_t)stream);
    }
    if (!x) return fail(-1, "avc_forward_ragged: null argument");
    if (p->flags & AVC_PLAN_CONTENT_ONLY)   // (the content encoder alone: x_cond is ignored, the result is ws["muls"])
        return rag_forward_impl(p, params, x, nullptr, nullptr, 0, 0, nullptr, 0, ws, (hipStream_t)stream);
    if (!x_cond) x_cond = x;
    return rag_forward_impl(p, params, x, x_cond, nullptr, 0, 0, nullptr, 0, ws, (hipStream_t)stream);
}

// conversion from embeddings the caller already has (an enrolled speaker, a mean, a point between two speakers)
extern "C" int avc_forward_ragged_emb(const avc_plan* p, const float* params, const float* x, const float* emb, long seb, long sec, float* ws,
                                      void* stream) {
    if (!p || !params || !x || !ws) return fail(-1, "avc_forward_ragged_emb: null argument");
    if ((p->flags & AVC_PLAN_RAGGED) && (p->flags & AVC_PLAN_DECODER_ONLY))
        return fail(-8, "avc_forward_ragged_emb: decoder-only ragged plans run through avc_decoder_forward_ragged");
    if ((p->flags & AVC_PLAN_RAGGED) && (p->flags & AVC_PLAN_CONTENT_ONLY))
        return fail(-8, "avc_forward_ragged_emb: content-only ragged plans run through avc_forward_ragged");
    if (!(p->flags & AVC_PLAN_RAGGED) || !(p->flags & AVC_PLAN_EMB_INPUT))
        return fail(-8, "avc_forward_ragged_emb: the plan was not created by avc_plan_create_ragged_ex with AVC_PLAN_EMB_INPUT");
    if (!emb) return fail(-1, "avc_forward_ragged_emb: emb is NULL (the plan has no speaker encoder to compute it)");
    if (int rc = check_row_strides("avc_forward_ragged_emb", "emb", p->Nd, p->cfg.dec.c_cond, seb, sec)) return rc;
    return rag_forward_impl(p, params, x, nullptr, emb, seb, sec, nullptr, 0, ws, (hipStream_t)stream);
}

// Decoder.forward over latents of different lengths (decoder-only fan-out plans): block s of z is [zc][Tz[s]] at float offset
// zc * offz[s]; its first c_in channels are the latent (zc = 2 c_out: the (mu | log_sigma) blocks a content plan leaves in ws["muls"])
extern "C" int avc_decoder_forward_ragged(const avc_plan* p, const float* params, const float* z, int zc, const float* emb, long seb, long sec,
                                          float* ws, void* stream) {
    if (!p || !params || !z || !ws) return fail(-1, "avc_decoder_forward_ragged: null argument");
    if (!(p->flags & AVC_PLAN_RAGGED) || !(p->flags & AVC_PLAN_DECODER_ONLY)) {
        if ((p->flags & AVC_PLAN_RAGGED) && (p->flags & AVC_PLAN_EMB_INPUT))
            return fail(-8, "avc_decoder_forward_ragged: the plan has a content encoder, it runs through avc_forward_ragged_emb");
        if (p->flags & AVC_PLAN_RAGGED) return fail(-8, "avc_decoder_forward_ragged: the plan runs through avc_forward_ragged");
        return fail(-8, "avc_decoder_forward_ragged: not a ragged plan (uniform decoder plans run through avc_decoder_forward)");
    }
    if (!emb) return fail(-1, "avc_decoder_forward_ragged: emb is NULL (the plan has no speaker encoder to compute it)");
    if (zc < p->cfg.dec.c_in)
        return fail(-1, "avc_decoder_forward_ragged: zc is too small: a latent block has at least c_in rows (c_in: mu alone, 2 c_out: ws[\"muls\"] blocks)");
    if (int rc = check_row_strides("avc_decoder_forward_ragged", "emb", p->Nd, p->cfg.dec.c_cond, seb, sec)) return rc;
    return rag_forward_impl(p, params, nullptr, nullptr, emb, seb, sec, z, zc, ws, (hipStream_t)stream);
}

// What the ragged backward passes share: where they run, and the plan's two ping-pong pairs of gradient rows.
struct RagBwd {
    const avc_plan* p;
    float* ws;
    const int* tab;
    hipStream_t s;
    float slope;
    float *gA, *gC;     // G_l = d(loss)/d(out_l), the residual path's gradient, and its next value
    float *dyA, *dyB;   // the rows entering a block's two input-gradient launches
    RagBwd(const avc_plan* p_, float* ws_, hipStream_t s_, float slope_)
        : p(p_), ws(ws_), tab((const int*)(ws_ + p_->rag_tab)), s(s_), slope(slope_), gA(ws_ + p_->gA2), gC(ws_ + p_->gC2), dyA(ws_ + p_->gA),
          dyB(ws_ + p_->gB) {}
    int launch(const ConvArgs& a) const { return avc_launch_conv(a, s, 11, p->tun); }
};

// An input-gradient launch on packed rows: dy of level `sl` -> dx of level `ol` (tiles run over `ol`)
// (always the 64 x 64 tile: a ragged tile is one sample's 64 frames, the mirrored instances exist on that tile only)
static ConvArgs rag_dgrad(const RagBwd& c, const LayerP& L, const float* dy, const avc_plan::RagLevel& sl, int cx, float* dx,
                          const avc_plan::RagLevel& ol, int cout) {
    ConvArgs a = mk_dgrad(c.slope, L, c.ws, dy, 0, -1, 1, 1, 1, 0, 64, dx, 0, 0, 1);
    set_rag(a, c.tab, sl, cx, ol, ol, cout);
    return a;
}

// InstanceNorm backward over the n samples' [C][T_b] rows of level l: g -> dy, from the saved rows at y and their statistics at st.
// coff >= 0: AdaIN with the decoder's cond slice at coff (its d(cond) slice is written too); up: planar store factor.  coff < 0: plain.
static int rag_in_bwd(const RagBwd& c, int n, int C, const float* g, long y, long st, const avc_plan::RagLevel& l, float* dy, int coff = -1,
                      int up = 1) {
    const DecNet& d = c.p->dec;
    RagINBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.g = g; a.y = c.ws + y; a.mean = c.ws + st; a.rstd = c.ws + st + (long)n * C; a.dy = dy;
    a.T = c.tab + l.dT; a.off = c.tab + l.doff;
    a.B = n; a.C = C; a.slope = c.slope;
    if (coff >= 0) { a.cond = c.ws + d.cond; a.dcond = c.ws + d.dcond; a.cond_sb = (long)2 * d.n * 2 * C; a.cond_off = coff; a.up = up; }
    return avc_launch_rag_in_bwd(a, c.s);
}

// The end of an encoder's input gradient, from dy = d(loss)/d(in_conv's output):
//   d(cat) for the bank channels, masked by the bank's activations (cat > 0), then
//   d(x) = W_in[:, nb c_bank:]^T dy + sum_g pad_g^T(bank_g^T(dcat_g)): nb + 1 launches, each after the first adds the running sum through
//   its residual join, in place -- a fixed order.  Stored as [T_b][M] rows, x's own layout, at e.dx.
static int rag_enc_input_tail(const RagBwd& c, const EncNet& e, const avc_plan::RagLevel& l0, const float* dy) {
    const avc_plan* p = c.p;
    const int C = e.c.c_h, M = e.c.c_in;
    {
        ConvArgs a = rag_dgrad(c, p->layers[e.in_conv], dy, l0, C, nullptr, l0, e.CC);
        a.g[0].out2 = c.ws + e.dcat;
        a.g[0].mask = c.ws + e.cat;
        RUN(c.launch(a));
    }
    float* dx = c.ws + e.dx;
    {
        ConvArgs a = rag_dgrad(c, p->layers[e.in_pass], dy, l0, C, dx, l0, M);
        a.oc = 1; a.ot = M;
        RUN(c.launch(a));
    }
    for (int g = 0; g < e.nb; ++g) {
        ConvArgs a = rag_dgrad(c, p->layers[e.bank[g]], c.ws + e.dcat, l0, e.CC, dx, l0, M);
        a.rag.xc0 = g * e.c.c_bank;
        a.oc = 1; a.ot = M;
        set_rag_res(a, c.tab, dx, AVC_RES_IDENTITY, l0, M);
        a.rc = 1; a.rt = M;
        RUN(c.launch(a));
    }
    return 0;
}

// The backward pass of a ragged speaker plan with AVC_PLAN_INPUT_GRADS: d(loss)/d(x_cond) from d(loss)/d(emb), parameters frozen.
// One branch on the caller's stream, the uniform speaker branch of avc_backward_impl minus every weight gradient:
//   d_emb -> [c_out][B] -> dense-stack backward -> d(pooled) -> pooling adjoint over each row's own length -> per block the two
//   input-gradient launches (ragged instances of conv_gemm_kernel; the pool adjoint of the residual path rides in the second one's
//   epilogue) -> in_conv input gradient (d(cat), masked by the bank's activations) -> the nb + 1 terms of d(x_cond), summed through the
//   residual join of consecutive launches into ws["d_x_cond"] in x_cond's own [sum T][M] layout.
// avc_backward_ragged_params only (grads == NULL: the frozen pass records nothing): a layer's dy was just produced and its forward input is
// saved -> one job of the next ragged weight-gradient launch (conv_wgrad_ragged.hip).  launch() goes out behind the phase that produced the
// dy rows and before the ping-pong rows are overwritten; layers that were split leave partial slots, which ONE reduce launch at the end of
// the pass sums in slot order into the flat gradient buffer.
struct RagWg {
    const avc_plan* p;
    float* ws;
    float* grads;
    const int* tab;
    hipStream_t s;
    std::vector<RagWgJob> jobs;
    std::vector<RagWgRed> reds;
    // x: blocks of xC channels on level xl, the layer reads Cin of them from xc0; dy: blocks of dyC channels on level yl, Cout from dyc0
    // k: which tensor of a stacked layer (its L.rows output channels lie at dyc0 + k L.rows of the dy blocks); every other layer: k = 0
    void add(const LayerP& L, const float* x, int xC, int xc0, const avc_plan::RagLevel& xl, const float* dy, int dyC, int dyc0,
             const avc_plan::RagLevel& yl, int k = 0) {
        if (!grads) return;
        RagWgJob j;
        memset(&j, 0, sizeof(j));
        j.x = x; j.dy = dy;
        j.Tin = tab + xl.dT; j.offin = tab + xl.doff; j.Tout = tab + yl.dT; j.offout = tab + yl.doff; j.chunk = tab + yl.dchunk;
        j.xC = xC; j.xc0 = xc0; j.dyC = dyC; j.dyc0 = dyc0 + k * L.rows;
        j.Cin = L.Cin; j.Cout = L.rows; j.KS = L.KS; j.stride = L.stride;
        j.nchunks = yl.nchunks;
        finish(j, L, k);
    }
    // tensor k of a stacked Linear over N rows read through strides (RagWgJob::strided): x(n, ci) = x[n sxn + ci sxc], dy likewise
    void add_strided(const LayerP& L, int k, const float* x, long sxn, long sxc, const float* dy, long syn, long syc, int N) {
        if (!grads) return;
        RagWgJob j;
        avc_rwg_strided_job(j, x, sxn, sxc, dy, syn, syc, N, L.Cin, L.rows);
        finish(j, L, k);
    }
    // where the job's result goes: straight into grads, or into the layer's slots and through the reduce launch
    void finish(RagWgJob& j, const LayerP& L, int k) {
        j.nsplit = L.rwg_nsplit;
        j.slot_floats = avc_rwg_slot_floats(L.Cin, L.rows, L.KS);
        float* dw = grads + p->params[L.w[k]].off;
        float* db = grads + p->params[L.b[k]].off;
        j.out = j.nsplit > 1 ? ws + L.rwg_slab + (long)k * j.nsplit * j.slot_floats : dw;
        j.db = db;
        jobs.push_back(j);
        if (j.nsplit > 1) {
            RagWgRed r;
            memset(&r, 0, sizeof(r));
            r.slab = j.out; r.dw = dw; r.db = db;
            r.slot_floats = j.slot_floats; r.n_w = (long)L.rows * L.Cin * L.KS; r.n_b = L.rows; r.nsplit = j.nsplit;
            reds.push_back(r);
        }
    }
    int launch() {
        if (jobs.empty()) return 0;
        const int rc = avc_launch_rwg(jobs.data(), (int)jobs.size(), s);
        jobs.clear();
        return rc;
    }
    int reduce() { return reds.empty() ? 0 : avc_launch_rwg_reduce(reds.data(), (int)reds.size(), s); }
};

static int rag_backward_impl(const avc_plan* p, const float* d_emb, long seb, long sec, float* ws, hipStream_t s, float* grads = nullptr) {
    const int B = p->B;
    const EncNet& e = p->spk;
    const std::vector<avc_plan::RagLevel>& lv = p->rl_spk;
    const int C = e.c.c_h;
    RagBwd c(p, ws, s, e.slope);
    const int* tab = c.tab;
    RagWg w{p, ws, grads, tab, s, {}, {}};
    RUN(avc_launch_transpose_strided(ws + p->demb, d_emb, seb, sec, B, e.c.c_out, s));
    float* dhA = ws + p->dhA;
    {
        DenseArgs da = dense_stack_args(p, e, nullptr, ws, true);
        da.in = ws + p->demb;
        da.dpooled = dhA;
        for (int l = 0; l < da.nlayers - 1; ++l) da.layer[l].dz = ws + (grads ? p->rag_dz[l] : p->dz);
        RUN(avc_launch_dense(da, 1, s));
        if (grads) {   // the 2 nd + 1 Linears: x and dz are [C][B] channel-major rows, ONE sample of B frames to the ragged kernel
            const avc_plan::RagLevel& ld = p->rl_dense;
            w.add(p->layers[e.outl], ws + e.hd[e.nd], C, 0, ld, ws + p->demb, e.c.c_out, 0, ld);
            for (int l = e.nd - 1; l >= 0; --l) {
                w.add(p->layers[e.dn2[l]], ws + e.d1[l], C, 0, ld, ws + p->rag_dz[2 * l + 1], C, 0, ld);
                w.add(p->layers[e.dn1[l]], ws + e.hd[l], C, 0, ld, ws + p->rag_dz[2 * l], C, 0, ld);
            }
            RUN(w.launch());
        }
    }
    RUN(avc_launch_rag_timepool_bwd(dhA, ws + e.a2[e.n - 1], tab + lv[e.n].dT, tab + lv[e.n].doff, B, C, lv[e.n].off[B], c.gA, c.dyA, c.slope, s));
    for (int l = e.n - 1; l >= 0; --l) {
        const int sub = e.c.subsample[l];
        {   // dyB = conv2^T(dyA) masked by a1
            ConvArgs a = rag_dgrad(c, p->layers[e.c2[l]], c.dyA, lv[l + 1], C, nullptr, lv[l], C);
            a.g[0].out2 = c.dyB;
            a.g[0].mask = ws + e.a1[l];
            RUN(c.launch(a));
        }
        // both dy rows of the block are live here and nowhere else: dW(conv2) = dyA x a1, dW(conv1) = dyB x out_l, one launch
        w.add(p->layers[e.c2[l]], ws + e.a1[l], C, 0, lv[l], c.dyA, C, 0, lv[l + 1]);
        w.add(p->layers[e.c1[l]], ws + e.out[l], C, 0, lv[l], c.dyB, C, 0, lv[l]);
        RUN(w.launch());
        {   // G_l = conv1^T(dyB) + pool^T(G_{l+1}); dyA = G_l masked by the activation that produced out_l
            ConvArgs a = rag_dgrad(c, p->layers[e.c1[l]], c.dyB, lv[l], C, l > 0 ? c.gC : nullptr, lv[l], C);
            set_rag_res(a, tab, c.gA, sub > 1 ? AVC_RES_POOLT : AVC_RES_IDENTITY, lv[l + 1], C);
            a.g[0].out2 = c.dyA;
            a.g[0].mask = (l > 0) ? ws + e.a2[l - 1] : ws + e.h0;
            RUN(c.launch(a));
        }
        std::swap(c.gA, c.gC);
    }
    RUN(rag_enc_input_tail(c, e, lv[0], c.dyA));
    if (!grads) return 0;
    // d(cat) and cat hold the in_conv's and all bank members' operands at once: dW(in_conv) = dyA x cat, dW(bank g) = its slice of d(cat) x
    // the M pass-through rows of cat (x itself) -- one launch; then every split layer's slots -> grads
    w.add(p->layers[e.in_conv], ws + e.cat, e.CC, 0, lv[0], c.dyA, C, 0, lv[0]);
    for (int g = 0; g < e.nb; ++g)
        w.add(p->layers[e.bank[g]], ws + e.cat, e.CC, e.nb * e.c.c_bank, lv[0], ws + e.dcat, e.CC, g * e.c.c_bank, lv[0]);
    RUN(w.launch());
    return w.reduce();
}

// The ragged speaker backward WITH parameter gradients: rag_backward_impl plus one ragged weight-gradient launch behind each phase that
// produces a layer's dy (the dense stack; each block; the in_conv and the bank together) and one reduce launch: 1 + n + 1 + 1 launches on
// top of the frozen pass.  Overwrites exactly the speaker encoder's tensors of `grads`.
extern "C" int avc_backward_ragged_params(const avc_plan* p, const float* params, const float* x_cond, const float* d_emb, long seb, long sec,
                                          float* grads, float* ws, void* stream) {
    if (!p || !params || !x_cond || !d_emb || !grads || !ws)
        return fail(-1, "avc_backward_ragged_params: null argument (pass the plan, params, x_cond and workspace of the avc_forward_ragged this pass follows, d_emb [B, c_cond] and grads)");
    if (!(p->flags & AVC_PLAN_RAGGED) || !(p->flags & AVC_PLAN_SPEAKER_ONLY) || !(p->flags & AVC_PLAN_INPUT_GRADS) || !(p->flags & AVC_PLAN_PART_GRADS))
        return fail(-8, "avc_backward_ragged_params: the plan was not created by avc_plan_create_ragged_speaker_grads");
    if (p->compute != AVC_COMPUTE_F32)
        return fail(-8, "avc_backward_ragged_params: the avc_plan_create_ragged_speaker_grads plan computes with bf16 operand rounding, a forward-only model; "
                        "gradients need fp32 (avc_plan_set_compute_dtype(p, 0)) or a uniform plan");
    if (int rc = check_row_strides("avc_backward_ragged_params", "d_emb", p->B, p->cfg.dec.c_cond, seb, sec)) return rc;
    return rag_backward_impl(p, d_emb, seb, sec, ws, (hipStream_t)stream, grads);
}

extern "C" int avc_backward_ragged(const avc_plan* p, const float* params, const float* x_cond, const float* d_emb, long seb, long sec, float* ws,
                                   void* stream) {
    if (!p || !params || !x_cond || !d_emb || !ws)
        return fail(-1, "avc_backward_ragged: null argument (pass the plan, params, x_cond and workspace of the avc_forward_ragged this pass follows, and d_emb [B, c_cond])");
    if (!(p->flags & AVC_PLAN_RAGGED) || !(p->flags & AVC_PLAN_SPEAKER_ONLY) || !(p->flags & AVC_PLAN_INPUT_GRADS))
        return fail(-8, "avc_backward_ragged: the plan was not created by avc_plan_create_ragged_ex with AVC_PLAN_SPEAKER_ONLY | AVC_PLAN_INPUT_GRADS");
    if (p->compute != AVC_COMPUTE_F32)
        return fail(-8, "avc_backward_ragged: the plan computes with bf16 operand rounding, a forward-only model; gradients need the fp32 compute dtype "
                        "(avc_plan_set_compute_dtype(p, 0)) or a uniform plan");
    if (int rc = check_row_strides("avc_backward_ragged", "d_emb", p->B, p->cfg.dec.c_cond, seb, sec)) return rc;
    return rag_backward_impl(p, d_emb, seb, sec, ws, (hipStream_t)stream);
}

// The backward pass of a plan of avc_plan_create_ragged_content_grads: d(loss)/d(x) from d(loss)/d(mu | log_sigma), parameters frozen.  One
// branch on the caller's stream, the uniform content branch of avc_backward_impl minus every weight gradient:
//   d_muls -> heads^T -> per block, last to first: IN-bwd(y2) -> conv2^T -> IN-bwd(y1) -> conv1^T with the pool / identity adjoint of the
//   residual path in its epilogue join -> IN-bwd(y0) -> in_conv input gradient (d(cat), masked by the bank's activations) -> the nb + 1 terms
//   of d(x), summed through the residual join of consecutive launches into ws["d_x"] in x's own [sum T][M] layout (as rag_backward_impl).
// avc_content_backward_ragged_params only (grads == NULL: the frozen pass records nothing and launches what it launched): the RagWg jobs
// of rag_backward_impl.  conv1's dy of a block goes to the plan's extra row set dy1 instead of dyA, so conv2's dy (dyA) is still live
// behind it and the block's two jobs share ONE launch (the alternative, launching conv2's job before the second InstanceNorm backward,
// costs n more launches); the two heads' jobs read the caller's d_muls and ride in the first block's launch.
static int rag_content_backward_impl(const avc_plan* p, const float* d_muls, float* ws, hipStream_t s, float* grads = nullptr) {
    const int B = p->B;
    const EncNet& e = p->enc;
    const std::vector<avc_plan::RagLevel>& lv = p->rl_enc;
    const int C = e.c.c_h;
    RagBwd c(p, ws, s, e.slope);
    RagWg w{p, ws, grads, c.tab, s, {}, {}};
    float* dy1 = grads ? ws + p->rag_dy1 : c.dyA;
    {   // G_n = heads^T(d_muls): the caller's [2 c_out][Tz_s] blocks
        ConvArgs a = rag_dgrad(c, p->layers[e.heads], d_muls, lv[e.n], 2 * e.c.c_out, c.gA, lv[e.n], C);
        RUN(c.launch(a));
    }
    for (int k = 0; k < 2; ++k)   // mean_layer, std_layer: rows [k c_out, (k + 1) c_out) of the d_muls blocks
        w.add(p->layers[e.heads], ws + e.out[e.n], C, 0, lv[e.n], d_muls, 2 * e.c.c_out, 0, lv[e.n], k);
    for (int l = e.n - 1; l >= 0; --l) {
        const int sub = e.c.subsample[l];
        RUN(rag_in_bwd(c, B, C, c.gA, e.y2[l], e.st2[l], lv[l + 1], c.dyA));
        {   // d(a1) = conv2^T(d(y2))
            ConvArgs a = rag_dgrad(c, p->layers[e.c2[l]], c.dyA, lv[l + 1], C, c.dyB, lv[l], C);
            RUN(c.launch(a));
        }
        RUN(rag_in_bwd(c, B, C, c.dyB, e.y1[l], e.st1[l], lv[l], dy1));
        // dW(conv2) = d(y2) x a1, dW(conv1) = d(y1) x out_l: one launch
        w.add(p->layers[e.c2[l]], ws + e.a1[l], C, 0, lv[l], c.dyA, C, 0, lv[l + 1]);
        w.add(p->layers[e.c1[l]], ws + e.out[l], C, 0, lv[l], dy1, C, 0, lv[l]);
        RUN(w.launch());
        {   // G_l = conv1^T(d(y1)) + pool^T(G_{l+1})
            ConvArgs a = rag_dgrad(c, p->layers[e.c1[l]], dy1, lv[l], C, c.gC, lv[l], C);
            set_rag_res(a, c.tab, c.gA, sub > 1 ? AVC_RES_POOLT : AVC_RES_IDENTITY, lv[l + 1], C);
            RUN(c.launch(a));
        }
        std::swap(c.gA, c.gC);
    }
    RUN(rag_in_bwd(c, B, C, c.gA, e.h0, e.st0, lv[0], c.dyA));
    RUN(rag_enc_input_tail(c, e, lv[0], c.dyA));
    if (!grads) return 0;
    // as the speaker pass: dW(in_conv) = d(y0) x cat, dW(bank g) = its slice of d(cat) x the M pass-through rows of cat; then the slots -> grads
    w.add(p->layers[e.in_conv], ws + e.cat, e.CC, 0, lv[0], c.dyA, C, 0, lv[0]);
    for (int g = 0; g < e.nb; ++g)
        w.add(p->layers[e.bank[g]], ws + e.cat, e.CC, e.nb * e.c.c_bank, lv[0], ws + e.dcat, e.CC, g * e.c.c_bank, lv[0]);
    RUN(w.launch());
    return w.reduce();
}

extern "C" int avc_content_backward_ragged(const avc_plan* p, const float* params, const float* x, const float* d_muls, float* ws, void* stream) {
    if (!p || !params || !x || !d_muls || !ws)
        return fail(-1, "avc_content_backward_ragged: null argument (pass the avc_plan_create_ragged_content_grads plan, params, x and workspace of the avc_forward_ragged this pass follows, and d_muls)");
    if (!(p->flags & AVC_PLAN_RAGGED) || !(p->flags & AVC_PLAN_CONTENT_ONLY) || !(p->flags & AVC_PLAN_INPUT_GRADS))
        return fail(-8, "avc_content_backward_ragged: the plan was not created by avc_plan_create_ragged_content_grads");
    if (p->compute != AVC_COMPUTE_F32)
        return fail(-8, "avc_content_backward_ragged: the avc_plan_create_ragged_content_grads plan computes with bf16 operand rounding, a forward-only model; "
                        "gradients need fp32 (avc_plan_set_compute_dtype(p, 0)) or a uniform plan");
    return rag_content_backward_impl(p, d_muls, ws, (hipStream_t)stream);
}

// The ragged content backward WITH parameter gradients: rag_content_backward_impl plus one ragged weight-gradient launch per block (the
// heads in the first), one for the in_conv and the bank, and one reduce launch: n + 2 launches on top of the frozen pass.  Overwrites
// exactly the content encoder's tensors of `grads`.
extern "C" int avc_content_backward_ragged_params(const avc_plan* p, const float* params, const float* x, const float* d_muls, float* grads,
                                                  float* ws, void* stream) {
    if (!p || !params || !x || !d_muls || !grads || !ws)
        return fail(-1, "avc_content_backward_ragged_params: null argument (pass the avc_plan_create_ragged_content_param_grads plan, params, x and workspace of the avc_forward_ragged this pass follows, d_muls and grads)");
    if (!(p->flags & AVC_PLAN_RAGGED) || !(p->flags & AVC_PLAN_CONTENT_ONLY) || !(p->flags & AVC_PLAN_INPUT_GRADS) || !(p->flags & AVC_PLAN_PART_GRADS))
        return fail(-8, "avc_content_backward_ragged_params: the plan was not created by avc_plan_create_ragged_content_param_grads");
    if (p->compute != AVC_COMPUTE_F32)
        return fail(-8, "avc_content_backward_ragged_params: the avc_plan_create_ragged_content_param_grads plan computes with bf16 operand rounding, a forward-only model; "
                        "gradients need fp32 (avc_plan_set_compute_dtype(p, 0)) or a uniform plan");
    return rag_content_backward_impl(p, d_muls, ws, (hipStream_t)stream, grads);
}

// The backward pass of a plan of avc_plan_create_ragged_decoder_grads: d(loss)/d(z) and d(loss)/d(emb) from d(loss)/d(dec), parameters
// frozen.  One branch on the caller's stream, the uniform decoder chain of avc_backward_impl minus every weight gradient:
//   d_dec -> out_conv^T -> per block, last to first: AdaIN-bwd(y2) (planar store where the block upsamples: the rows leave as the conv's
//   own [C up][T_l] output rows) -> conv2^T -> AdaIN-bwd(y1) -> conv1^T with the nearest-upsampling / identity adjoint of the residual path
//   in its epilogue join -> IN-bwd(y0) -> in_conv^T into ws["d_z"] ([c_in][Tz_s] blocks) -> d(emb) = W_affine^T d(cond), one uniform
//   input-gradient launch over N columns that stores row-major [N][c_cond] into ws["d_emb"].
// 1 + 4 n + 2 + 1 launches (28 for the stock 6 blocks): every AdaIN backward writes its [N][2 C] slice of d(cond) once, nothing is zeroed.
// avc_decoder_backward_ragged_params only (grads == NULL: the frozen pass records nothing, launches what it launched and reads neither z
// nor emb): the RagWg jobs, with conv1's dy in the plan's extra row set as in rag_content_backward_impl.  out_conv's job reads the caller's
// d_dec and rides in the last block's launch; conv2's dy is already planar -- the conv's own [C up][T_l] output rows -- so its job is a
// packed one on level l; the in_conv's job (KS = 1) reads the caller's latent blocks in place; the 2n affine Linears are 2n STRIDED jobs
// (dy = the [N][2 C] slice of frame-major d(cond), x = the caller's emb through (seb, sec)) in the in_conv's launch.
static int rag_decoder_backward_impl(const avc_plan* p, const float* d_dec, float* ws, hipStream_t s, float* grads = nullptr, const float* z = nullptr,
                                     int zc = 0, const float* emb = nullptr, long seb = 0, long sec = 0) {
    const int N = p->Nd;
    const DecNet& d = p->dec;
    const std::vector<avc_plan::RagLevel>& lv = p->rl_dec;
    const int C = d.c.c_h, Cz = d.c.c_in;
    const long csb = (long)2 * d.n * 2 * C;
    RagBwd c(p, ws, s, d.slope);
    RagWg w{p, ws, grads, c.tab, s, {}, {}};
    float* dy1 = grads ? ws + p->rag_dy1 : c.dyA;
    {   // G_n = out_conv^T(d_dec): the caller's [M][T''_j] blocks
        ConvArgs a = rag_dgrad(c, p->layers[d.out_conv], d_dec, lv[d.n], p->M, c.gA, lv[d.n], C);
        RUN(c.launch(a));
    }
    w.add(p->layers[d.out_conv], ws + d.out[d.n], C, 0, lv[d.n], d_dec, p->M, 0, lv[d.n]);
    for (int l = d.n - 1; l >= 0; --l) {
        const int up = d.c.upsample[l];
        RUN(rag_in_bwd(c, N, C, c.gA, d.y2[l], d.st2[l], lv[l + 1], c.dyA, (2 * l + 1) * 2 * C, up));
        {   // d(a1) = conv2^T(d(y2)): d(y2) lies as the conv's own output rows [C up][T_l] (C up off_l == C off_{l+1}: the same block starts)
            ConvArgs a = rag_dgrad(c, p->layers[d.c2[l]], c.dyA, lv[l], C * up, c.dyB, lv[l], C);
            RUN(c.launch(a));
        }
        RUN(rag_in_bwd(c, N, C, c.dyB, d.y1[l], d.st1[l], lv[l], dy1, (2 * l) * 2 * C, 1));
        // dW(conv2) = d(y2) x a1 (both on level l), dW(conv1) = d(y1) x out_l: one launch
        w.add(p->layers[d.c2[l]], ws + d.a1[l], C, 0, lv[l], c.dyA, C * up, 0, lv[l]);
        w.add(p->layers[d.c1[l]], ws + d.out[l], C, 0, lv[l], dy1, C, 0, lv[l]);
        RUN(w.launch());
        {   // G_l = conv1^T(d(y1)) + up^T(G_{l+1})
            ConvArgs a = rag_dgrad(c, p->layers[d.c1[l]], dy1, lv[l], C, c.gC, lv[l], C);
            set_rag_res(a, c.tab, c.gA, up > 1 ? AVC_RES_UPT : AVC_RES_IDENTITY, lv[l + 1], C);
            RUN(c.launch(a));
        }
        std::swap(c.gA, c.gC);
    }
    RUN(rag_in_bwd(c, N, C, c.gA, d.y0, d.st0, lv[0], c.dyA));
    {   // d(z): blocks [c_in][Tz_s] at c_in * offz[s]
        ConvArgs a = rag_dgrad(c, p->layers[d.in_conv], c.dyA, lv[0], C, ws + p->dz, lv[0], Cz);
        RUN(c.launch(a));
    }
    {   // d(emb)[b][i] = sum_o W[o][i] d(cond)[b][o]: the stacked affine layer's input gradient, "frames" = the N samples (d(cond) read with
        // channel stride 1, frame stride csb), stored row-major through the output strides -- the mirror image of the forward affine launch
        ConvArgs a = mk_dgrad(c.slope, p->layers[d.affine], ws, ws + d.dcond, 0, 1, (int)csb, 1, 1, N, N, ws + p->demb_rm, 0, 1, d.c.c_cond);
        RUN(avc_launch_conv(a, s, 0, p->tun));
    }
    if (!grads) return 0;
    w.add(p->layers[d.in_conv], z, zc, 0, lv[0], c.dyA, C, 0, lv[0]);
    for (int k = 0; k < 2 * d.n; ++k)   // affine Linear k: beta rows, then gamma rows, as its AdaIN backward left them in d(cond)
        w.add_strided(p->layers[d.affine], k, emb, seb, sec, ws + d.dcond + (long)k * 2 * C, csb, 1, N);
    RUN(w.launch());
    return w.reduce();
}

// z / zc / emb / seb / sec: what the avc_decoder_forward_ragged this pass follows was given (the frozen-parameter pass reads the saved rows,
// not the inputs; they are checked like the forward's).  d_dec: packed [M][T''_j] blocks, the layout avc_plan_ragged_out reports (block j at
// M * sum of the output lengths before it).  Results: ws["d_z"] (blocks [c_in][Tz_s] at c_in * offz[s]) and ws["d_emb"] ([N][c_cond],
// always dense).  Allocates nothing, synchronises nothing: every launch goes to the caller's stream.
extern "C" int avc_decoder_backward_ragged(const avc_plan* p, const float* params, const float* z, int zc, const float* emb, long seb, long sec,
                                           const float* d_dec, float* ws, void* stream) {
    if (!p || !params || !z || !emb || !d_dec || !ws)
        return fail(-1, "avc_decoder_backward_ragged: null argument (pass the avc_plan_create_ragged_decoder_grads plan, params, z, emb and workspace of the "
                        "avc_decoder_forward_ragged this pass follows, and d_dec)");
    if (!(p->flags & AVC_PLAN_RAGGED) || !(p->flags & AVC_PLAN_INPUT_GRADS))
        return fail(-8, "avc_decoder_backward_ragged: the plan was not created by avc_plan_create_ragged_decoder_grads");
    if (p->flags & AVC_PLAN_FANOUT)
        return fail(-8, "avc_decoder_backward_ragged: fan-out plans (AVC_PLAN_FANOUT) have no decoder backward pass; create the plan with "
                        "avc_plan_create_ragged_decoder_grads (output j from latent j) and index the latents in the caller");
    if (!(p->flags & AVC_PLAN_DECODER_ONLY))
        return fail(-8, "avc_decoder_backward_ragged: the plan was not created by avc_plan_create_ragged_decoder_grads");
    if (p->compute != AVC_COMPUTE_F32)
        return fail(-8, "avc_decoder_backward_ragged: the avc_plan_create_ragged_decoder_grads plan computes with bf16 operand rounding, a forward-only model; "
                        "gradients need fp32 (avc_plan_set_compute_dtype(p, 0)) or a uniform plan (avc_decoder_backward)");
    if (zc < p->cfg.dec.c_in)
        return fail(-1, "avc_decoder_backward_ragged: zc is too small: a latent block has at least c_in rows");
    if (int rc = check_row_strides("avc_decoder_backward_ragged", "emb", p->Nd, p->cfg.dec.c_cond, seb, sec)) return rc;
    return rag_decoder_backward_impl(p, d_dec, ws, (hipStream_t)stream);
}

// The ragged decoder backward WITH parameter gradients: rag_decoder_backward_impl plus one ragged weight-gradient launch per block (out_conv
// in the first), one for the in_conv and the 2n affine Linears, and one reduce launch: n + 2 launches on top of the frozen pass.  z and emb
// are READ here (the in_conv's and the affine Linears' forward inputs): they must be the forward's.  Overwrites exactly the decoder's
// tensors of `grads`.
extern "C" int avc_decoder_backward_ragged_params(const avc_plan* p, const float* params, const float* z, int zc, const float* emb, long seb, long sec,
                                                  const float* d_dec, float* grads, float* ws, void* stream) {
    if (!p || !params || !z || !emb || !d_dec || !grads || !ws)
        return fail(-1, "avc_decoder_backward_ragged_params: null argument (pass the avc_plan_create_ragged_decoder_param_grads plan, params, z, emb and workspace of the "
                        "avc_decoder_forward_ragged this pass follows, d_dec and grads)");
    if (!(p->flags & AVC_PLAN_RAGGED) || !(p->flags & AVC_PLAN_DECODER_ONLY) || !(p->flags & AVC_PLAN_INPUT_GRADS) || !(p->flags & AVC_PLAN_PART_GRADS) ||
        (p->flags & AVC_PLAN_FANOUT))
        return fail(-8, "avc_decoder_backward_ragged_params: the plan was not created by avc_plan_create_ragged_decoder_param_grads");
    if (p->compute != AVC_COMPUTE_F32)
        return fail(-8, "avc_decoder_backward_ragged_params: the avc_plan_create_ragged_decoder_param_grads plan computes with bf16 operand rounding, a forward-only model; "
                        "gradients need fp32 (avc_plan_set_compute_dtype(p, 0)) or a uniform plan (avc_decoder_backward)");
    if (zc < p->cfg.dec.c_in)
        return fail(-1, "avc_decoder_backward_ragged_params: zc is too small: a latent block has at least c_in rows");
    if (int rc = check_row_strides("avc_decoder_backward_ragged_params", "emb", p->Nd, p->cfg.dec.c_cond, seb, sec)) return rc;
    return rag_decoder_backward_impl(p, d_dec, ws, (hipStream_t)stream, grads, z, zc, emb, seb, sec);
}
