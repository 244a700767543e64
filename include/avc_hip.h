/* libavc_hip.so — C ABI of the MI355X-native AdaIN-VC forward/backward engine.
 *
 * The reference (jjery2243542/adaptive_voice_conversion) has no FFI of its own:
 * its hot path sits behind the torch.nn.Module `AE` (model.py:373-395) and
 * `Solver.ae_step` (solver.py:81-97).  This header is the boundary a binding
 * for that path attaches to: plain pointers, sizes and a hipStream_t; no torch
 * types.  The Python mirror of `AE`/`Solver` in adaptive_voice_conversion_amd/
 * binds it with ctypes (see INTEGRATION.md for the stub a reference maintainer
 * would add).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless stated; tensors are fp32.
 *  - activations are [B, C, T] with explicit element strides where a view may
 *    be handed in (the collate view of data_utils.py:14-16 has strides (T*M, 1, M)).
 *  - scratch memory is a caller-owned workspace whose size the plan reports; the data-path entry points (avc_forward* / avc_loss /
 *    avc_backward / avc_clip_adam_step / avc_plan_pack_weights and every op-level call) never allocate, free or synchronise -- they only
 *    enqueue work (graph-capture safe).  Three exceptions, all outside the per-step path, stated here because earlier revisions of this
 *    header claimed there were none:
 *      (1) avc_plan_create* allocates a small DEVICE table (hipMalloc: the weight-image descriptors of avc_plan_pack_weights, a few KB)
 *          and fills it with a blocking hipMemcpy; avc_plan_destroy frees it.  Create plans outside captured / latency-critical regions.
 *      (2) the FIRST plan created on a device creates that device's three helper HIP streams (below); they live until the process ends.
 *      (3) avc_forward_ragged, avc_forward_ragged_emb and avc_decoder_forward_ragged upload their per-utterance length / offset / tile tables (a few KB) with
 *          hipMemcpyAsync from pageable host memory: the call may block the host until the copy is staged and is NOT graph-capture safe
 *          (the uniform entry points are).
 *  - return value: 0 = ok, < 0 = bad argument / unsupported shape,
 *    > 0 = hipError_t.  avc_last_error() describes the last failure.
 *  - the stream is always an argument (backward runs on PyTorch's autograd
 *    thread).  A plan overlaps independent branches on three helper HIP streams -- one "side" stream (the
 *    speaker-encoder branch, the decoder's second half-batch chain) and two low-priority weight-gradient streams -- and on events of
 *    its own (created by avc_plan_create*, destroyed by avc_plan_destroy); every entry point joins them back into the caller's stream
 *    before it returns.  The three helper STREAMS are ONE set per device, created by the first plan on that device, shared by every
 *    plan of the process and never destroyed (a second set lands on whatever hardware queues the runtime's round-robin has reached
 *    and was measured 1.8 - 2.4x slower: scripts/two_plans_probe.py).  The side stream's priority is the FIRST plan's
 *    avc_tuning.side_prio; later plans get that stream whatever they ask for (avc_plan_side_priority reports it).  ONE call per plan
 *    may be in flight on the host at a time (two host threads need two plans); two plans driven from two threads are functionally
 *    independent but share the helper streams, i.e. their side-branch / weight-gradient work is serialised stream by stream
 *    (tests/test_engine.py::test_two_plans_from_two_threads: results bit-equal to the serial runs).
 *  - the library has no process-wide mutable state that changes RESULTS or heuristics: the only process-lifetime objects are the helper
 *    streams above.  Launch heuristics and
 *    diagnostic switches are an `avc_tuning` value that a plan captures at
 *    creation (avc_plan_create_tuned); the op-level entry points at the end of
 *    this header read a THREAD-LOCAL avc_tuning that avc_set_tuning edits for
 *    the calling thread only (micro-benchmarks and kernel tests).  No
 *    environment variable is read by the LIBRARY.  (The Python loader, _lib.py, honours
 *    AVC_HIP_LIB = path of an alternative build of this library: which .so is loaded for
 *    same-box A/B measurements, never how it behaves.)
 *  - the gradient all-reduce of data-parallel training deliberately lives in
 *    the host framework (torch.distributed "nccl" = RCCL over xGMI):
 *    this library exposes where to cut (avc_plan_param_range) and when each
 *    part of the flat gradient buffer is final (avc_plan_stream_wait_grads).
 */
#ifndef AVC_HIP_H
#define AVC_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

#define AVC_MAX_BLOCKS 8

/* config.yaml:1-24 (SpeakerEncoder / ContentEncoder blocks; n_dense_blocks = 0 for the content encoder) */
typedef struct avc_encoder_cfg {
    int c_in, c_h, c_out, kernel_size, bank_size, bank_scale, c_bank, n_conv_blocks, n_dense_blocks;
    int subsample[AVC_MAX_BLOCKS];
    int act; /* config.yaml `act` (model.py:93-99 get_act): 0 = relu, 1 = lrelu (nn.LeakyReLU, slope 0.01) */
} avc_encoder_cfg;

/* config.yaml:25-36 (Decoder) */
typedef struct avc_decoder_cfg {
    int c_in, c_cond, c_h, c_out, kernel_size, n_conv_blocks;
    int upsample[AVC_MAX_BLOCKS];
    int act; /* 0 = relu, 1 = lrelu */
} avc_decoder_cfg;

typedef struct avc_model_cfg {
    avc_encoder_cfg spk; /* model.py:209-277 */
    avc_encoder_cfg enc; /* model.py:279-323 */
    avc_decoder_cfg dec; /* model.py:325-371 */
} avc_model_cfg;

typedef struct avc_plan avc_plan; /* host-side launch plan for one (B, T, T_cond) shape */

int avc_version(void);
const char* avc_last_error(void);

/* ---- plan (host only) -------------------------------------------------- */
/* T = frames of the content/source segment, T_cond = frames of the speaker
 * (target) segment; training uses T_cond == T (model.py:380-385), inference may
 * differ (model.py:387-391).  Fails (like the reference, a1 in SURVEY §8a) when a
 * reflect pad is not smaller than the length it pads. */
int avc_plan_create(const avc_model_cfg* cfg, int B, int T, int T_cond, avc_plan** out);
/* flags: AVC_PLAN_INFERENCE = forward only (AE.inference, model.py:387-391): no gradient / slab / dy buffers in
 * the workspace, avc_loss / avc_backward are refused; AVC_PLAN_SPEAKER_ONLY (implies INFERENCE unless AVC_PLAN_PART_GRADS is set) = only
 * the speaker encoder runs (AE.get_speaker_embeddings, model.py:393-395): T is ignored, the result is ws["emb"]. */
#define AVC_PLAN_INFERENCE 1
#define AVC_PLAN_SPEAKER_ONLY 2
/* PART PLANS: one of the three networks alone, the reference's sub-module calls (AE.forward / AE.inference are a few lines that call
 * them, model.py:380-395).  At most one part flag; each combines with AVC_PLAN_X3 / AVC_PLAN_BF16S / avc_plan_set_compute_dtype as a
 * whole plan does, and a branch runs the SAME kernel instances in a part plan as in a whole plan of that (B, T) (the launch choice is a
 * function of the layer and its shape only).  A part plan packs only its branch's weight images and allocates only its branch's buffers
 * (avc_plan_workspace_floats is smaller than a whole plan's); it still takes the full flat parameter buffer (same avc_plan_param_info)
 * and a backward writes exactly its branch's avc_plan_param_range (AVC_GRADS_SPEAKER / _CONTENT / _DECODER) of `grads`, nothing else.
 * Without AVC_PLAN_PART_GRADS a part plan is forward-only (implies AVC_PLAN_INFERENCE: no gradient buffers, backward refused);
 * avc_loss is refused on every part plan.  Nothing here allocates or synchronises beyond what avc_plan_create* does for any plan.
 *  - AVC_PLAN_SPEAKER_ONLY (SpeakerEncoder.forward, model.py:265-277): avc_forward(_ex) -> ws["emb"] [B, c_cond]; T is ignored.
 *    With PART_GRADS: avc_backward with d_emb_up only (d_dec, d_muls_up NULL).
 *  - AVC_PLAN_CONTENT_ONLY (ContentEncoder.forward, model.py:301-323): avc_forward(_ex) with x_cond and eps ignored -> ws["muls"]
 *    [B, 2 c_out, Tb] (mu | log_sigma).  With PART_GRADS: avc_backward with d_muls_up (d_dec, d_emb_up NULL); lambda_kl adds the KL
 *    term of solver.py:86-88 as for a whole plan.
 *  - AVC_PLAN_DECODER_ONLY (Decoder.forward, model.py:347-371): create with T = Tb, the latent length the caller supplies (T_cond is
 *    ignored; Tb must satisfy the decoder's reflect-pad rule); avc_plan_out_len = Tb * prod(upsample).  It runs through
 *    avc_decoder_forward / avc_decoder_backward below, never avc_forward / avc_backward. */
#define AVC_PLAN_CONTENT_ONLY 32
#define AVC_PLAN_DECODER_ONLY 64
#define AVC_PLAN_PART_GRADS 128
/* AVC_PLAN_INPUT_GRADS: avc_backward also computes the gradients with respect to the input spectrograms (the reference's x.grad when
 * x requires grad).  Combines with whole plans (not AVC_PLAN_INFERENCE) and with the speaker / content part plans that have
 * AVC_PLAN_PART_GRADS; refused with AVC_PLAN_DECODER_ONLY.  Adds to the plan: an input-gradient weight image of every conv-bank layer
 * (transposed, tap-flipped) and one of the in_conv's M pass-through input rows, per encoder that runs; one fp32 [B, M, T] buffer per
 * encoder.  After avc_backward:
 *  - ws["d_x"] [B, M, T] fp32 contiguous: d(loss)/d(x).  Whole plans called with x_cond NULL (one input read by both encoders,
 *    AE.forward) leave there the sum of both encoders' terms: content first, then speaker, in that fixed order.  With a non-NULL
 *    x_cond it is the content encoder's term alone -- also when x_cond points at the same memory as x.
 *  - ws["d_x_cond"] [B, M, T_cond] fp32 contiguous (whole plans): d(loss)/d(x_cond), the speaker encoder's term, when x_cond is not
 *    NULL (AE.inference(x, x_cond); T_cond may differ from T and eps may be NULL).
 * Speaker part plans leave their gradient in ws["d_x"].  Plans without the flag are unchanged (weight images, workspace, launches). */
#define AVC_PLAN_INPUT_GRADS 256
int avc_plan_create_ex(const avc_model_cfg* cfg, int B, int T, int T_cond, int flags, avc_plan** out);
int avc_plan_flags(const avc_plan* p);
/* priority class of the device's shared side stream this plan runs its side branch on: 1 = highest, 0 = normal, -1 = the plan has no
 * helper streams (no device at creation: every kernel goes to the caller's stream) */
int avc_plan_side_priority(const avc_plan* p);
void avc_plan_destroy(avc_plan* p);
/* flat parameter buffer: the 166 state_dict tensors in reference
 * registration order, each at a 16-byte aligned offset */
int avc_plan_num_params(const avc_plan* p);
long avc_plan_param_floats(const avc_plan* p);                                   /* total floats incl. padding */
int avc_plan_param_info(const avc_plan* p, int i, long* offset, long* numel, int dims[3]);
long avc_plan_workspace_floats(const avc_plan* p);
/* named workspace regions (float offsets): "muls" [B,2*c_out,Tb] (mu | log_sigma),
 * "emb" [B,c_cond], "dec" [B,M,T'], "z", "losses" [2], "grad_norm" [1], "d_dec", ... ; -1 if unknown */
long avc_plan_buffer(const avc_plan* p, const char* name);
int avc_plan_out_len(const avc_plan* p);    /* T' of dec: 8*ceil(T/8) for the stock config */
int avc_plan_latent_len(const avc_plan* p); /* Tb */

/* ReLU sites of the forward pass in the reference's call order (test/diagnostic aid: lets a checker
 * evaluate its own gradient on the SAME piecewise-linear branch the engine took).  kind 0: the
 * mask is (stored activation > 0) at ws[act_off] (strides sb, sc, st over [B, C, T]); kind 1
 * (InstanceNorm sites): the pre-activation is ((y - mean) * rstd) * gamma + beta with y at
 * ws[y_off] ([B,C,T] contiguous), mean/rstd at ws[stat_off] / ws[stat_off + B*C], and, when
 * cond_off >= 0, beta = ws[cond_off + b*cond_sb + c], gamma = ws[cond_off + b*cond_sb + C + c]. */
typedef struct avc_relu_site {
    int kind, B, C, T;
    long act_off, sb, sc, st;
    long y_off, stat_off, cond_off, cond_sb;
    long storage;   /* 0: fp32 tensors; AVC_PLAN_BF16S plans: 1 = bf16 pair tensor at act_off / y_off (dwords [B][C/2][T], sb / sc in dwords),
                     * 2 = natural bf16 rows [B][C][T] at y_off (the output of a pixel-shuffling conv) */
} avc_relu_site;
int avc_plan_num_relu_sites(const avc_plan* p);
int avc_plan_relu_site(const avc_plan* p, int i, avc_relu_site* out);

/* ---- data-parallel hooks: the flat gradient buffer is all-reduced by the caller (RCCL).
 * The backward pass finishes the decoder's parameter gradients first; they are the TAIL of the flat buffer.
 * avc_plan_param_range gives the float range of a part; avc_plan_stream_wait_grads makes `stream` wait until
 * that part, as written by the last avc_backward call on this plan, is final -- so the reduce of the decoder
 * range can run on a communication stream under the encoders' backward. */
#define AVC_GRADS_ALL 0
#define AVC_GRADS_DECODER 1
#define AVC_GRADS_ENCODERS 2
#define AVC_GRADS_SPEAKER 3   /* the speaker encoder's parameters (head of the flat buffer): final when its branch of the backward ends, */
#define AVC_GRADS_CONTENT 4   /* ... well before the content encoder's (the longer branch, InstanceNorm kernels in its chain) */
int avc_plan_param_range(const avc_plan* p, int part, long* offset, long* numel);
int avc_plan_stream_wait_grads(const avc_plan* p, int part, void* stream);

/* ---- launch heuristics and diagnostic switches (plan-scoped) ---------------------------------------------
 * avc_tuning_init fills the library defaults; a plan copies the struct at creation and never looks at the
 * caller's copy again.  Every field is an A/B-measurement or test aid: production code passes NULL. */
typedef struct avc_tuning {
    int struct_size;        /* sizeof(avc_tuning) of the caller (set by avc_tuning_init; a mismatch is refused) */
    int single_stream;      /* 1: every kernel on the caller's stream (profiling / per-class event brackets) */
    int dec_split_min;      /* smallest batch whose decoder forward AND backward run as two half-batch chains on two streams (128) */
    int conv_x3;            /* 1: split-bf16 conv kernel (csrc/conv_x3.hip) for the k = 5 layers that fill the chip; 2: every eligible layer */
    int wgrad_x3;           /* 1: split-bf16 products in the whole-chunk weight-gradient launches */
    int dgrad_par;          /* 0: stride-2 dgrad multiplies all taps of the zero-upsampled dy (default 1: one column parity per wave) */
    int bank_switch;        /* 0: generic run-time-taps chunk loop for the grouped bank launch / 1x1 convs (default 1) */
    int conv_ck5;           /* chunk depth of the k >= 4 convs at the op level: 8 (default) | 16 | 32 */
    int wgrad_batch;        /* weight gradients per batched launch (12) */
    int wgrad_batch_wgs;    /* workgroups a batched weight-gradient launch aims for (256) */
    int wgrad_target_wgs;   /* op level: split-K workgroups per weight-gradient launch (256) */
    int conv_ablation;      /* timing experiments only, WRONG results when set: bit0 no DMA, bit1 no MFMA, bit2 no barrier, bit3 no store */
    int wgrad_ablation;
    int op_compute_dtype;   /* op-level conv entry points: 0 fp32, 1 bf16 operands (plans: avc_plan_set_compute_dtype) */
    int side_prio;          /* 1 (default since round 5): the device's side stream (speaker-encoder branch, the longer pole of forward and backward) is
                             * created with the highest stream priority -- its kernels are dispatched ahead of the weight-gradient launches and the
                             * other branch's when CU slots free up (-2.2 % on the B = 256 step); 0: normal priority.  Honoured by the FIRST plan
                             * created on a device only: the helper streams are one set per device and process (see "Conventions") */
    int tile12_wgs;         /* 64 x 128 column tiles (two fragments per wave share each weight fragment) for stride-1 k = 5 layers whose launch still has
                             * at least this many workgroups; 0 = never */
    long wgrad_batch_units; /* pending (tile x K-chunk) units that trigger a batched launch early (1 << 40 = never) */
    long tile_thr11, tile_thr21, ck16_wgs, ck32_wgs, kg_wgs;   /* conv tile / chunk-depth / split-K-group thresholds in workgroups */
    long conv_min_lds;      /* occupancy experiment: every conv_gemm launch asks for at least this many BYTES of LDS (0 = what the tiles need) */
    long in_pairs_nv;       /* bf16 pair InstanceNorm rows: 16-byte vectors per lane, 1 (default: one lane group spans the row) | 2 | 4 */
    long bh_ck5;            /* AVC_PLAN_BF16S plans: chunk depth (DWORD channels = bf16 channel pairs) of the k >= 4 convs: 8 (default) | 16 | 32 */
    long wgrad_cw8;         /* 1: the weight gradients of the k = 5 layers (Cin % 64 == 0, Cout % 128 == 0) run on 128 x 64 tiles with EIGHT consumer
                             * waves (two MFMA waves per SIMD) + four producers.  0 (default): 64 x 64 tiles, four consumers.  Measured on MI355X,
                             * same box: the wgrad class is 2.21 vs 2.26 ms per step with it, the STEP 6.03 vs 5.98 ms (768 threads x 168 registers
                             * leave the chain's kernels no room on a CU the persistent workgroup sits on) */
    long dec_wgrad_flush;   /* decoder backward: every N recorded weight gradients go out at once, under the decoder's own (latency-bound) backward chain,
                             * as launches of only dec_wgrad_wgs persistent workgroups; 0 = all of them are held until the dense-stack backward
                             * kernel of the speaker branch has been launched (round 4's first schedule) */
    long dec_wgrad_wgs;     /* workgroups (= CUs occupied) of those early launches */
    long conv_walk;         /* conv_gemm tile walk (round 5, opt-in; exact-fp32 k = 5 / bank / 1x1 launches): a launch with at least conv_walk_min
                             * tiles per resident workgroup runs as PERSISTENT workgroups -- at most this many per CU (further bounded by LDS and
                             * registers) -- that each walk a list of column tiles, the next tile's first chunk in flight under the epilogue of
                             * this one.  Bit-identical results.  0 (default) = one tile per workgroup: measured no slower anywhere
                             * (profiles/r05_conv_walk_ablation.log).  < 0 (tests): exactly -conv_walk walkers per row slab */
    long conv_walk_min;     /* smallest number of tiles per walker worth a walk (2) */
    long conv_in_fuse;      /* 1: InstanceNorm / AdaIN / activation / residual of rows of 16 / 32 / 64 frames run inside the producing conv's epilogue
                             * (the 64-column tile holds whole rows; csrc/conv_shared.h: conv_epilogue_in) instead of a row kernel of their own */
    long dbg_streams;       /* diagnostic (scripts/bf16_repro_probe2.py): bit 0 = the backward pass launches its weight gradients on the stream that
                             * produced their operands (no weight-gradient streams); bit 1 = the backward pass runs the speaker branch and the
                             * decoder's second half-batch chain on the caller's stream (no side stream); bit 4 (16) = avc_plan_pack_weights packs image by image with
                             * the op-level gather kernel instead of the plan's one-launch table (tests/test_engine.py compares the two).  0 = the product schedule */
} avc_tuning;
void avc_tuning_init(avc_tuning* t);
/* avc_plan_create_ex with explicit tuning (NULL = defaults).  Additional flags: AVC_PLAN_X3 = compute mode "fp32x3"
 * (tuning->conv_x3 = 1, wgrad_x3 = 1 unless the caller's tuning already asks for more). */
#define AVC_PLAN_X3 4
#define AVC_PLAN_RAGGED 8   /* set by avc_plan_create_ragged (reported by avc_plan_flags) */
/* AVC_PLAN_BF16S = compute mode "bf16" with bf16 STORAGE (BASELINE configs[2]: bf16 compute, fp32 master weights and optimizer state):
 * every [B, C, T] activation and activation gradient in the workspace is a bf16 channel-pair tensor (dwords [B][C/2][T], see "bf16
 * PAIR storage" below), conv / Linear products run on v_mfma_f32_32x32x16_bf16 from bf16 pair weight images, accumulation, InstanceNorm
 * statistics, mu / log_sigma, dec, emb, the AdaIN affine parameters, all parameter gradients and the optimizer stay fp32.  Inputs and
 * outputs of the entry points keep their fp32 types.  Needs even channel counts and frame counts that are multiples of 4 at every level
 * (AVC_ERR_PAIR_SHAPE otherwise: a return code of its own, so that a caller can fall back to operand rounding -- avc_plan_set_compute_dtype(1) --
 * for THAT reason only); avc_plan_compute_dtype reports 3; avc_plan_buffer offsets of activation tensors then address pair tensors. */
#define AVC_PLAN_BF16S 16
#define AVC_ERR_PAIR_SHAPE (-12)
int avc_plan_create_tuned(const avc_model_cfg* cfg, int B, int T, int T_cond, int flags, const avc_tuning* tuning, avc_plan** out);
/* profiling aid on an existing plan: 1 = every kernel of this plan on the caller's stream */
int avc_plan_set_single_stream(avc_plan* p, int on);

/* Compute dtype of the Conv1d / Linear matrix products (BASELINE config 3: "bf16 compute, fp32 master
 * and optimizer state").  0 = fp32 MFMA, bit-exact fp32 arithmetic (default, the reference's precision);
 * 1 = operands rounded to bf16 (round-to-nearest-even) when they enter the matrix core, fp32 accumulate.
 * Parameters, activations, statistics, gradients and the optimizer stay fp32 in memory either way. */
int avc_plan_set_compute_dtype(avc_plan* p, int dtype);
int avc_plan_compute_dtype(const avc_plan* p);

/* ---- whole-model entry points (replace AE.forward / AE.inference, model.py:380-391) */
/* x: source mel [B,M,T]; x_cond: speaker mel [B,M,T_cond] (may alias x); eps: [B,c_out,Tb]
 * reparameterisation noise (model.py:383) or NULL for z = mu (AE.inference).
 * Results are left in the workspace regions "muls", "emb", "dec". */
int avc_forward(const avc_plan* p, const float* params, const float* x, long sxb, long sxc, int sxt,
                const float* x_cond, long scb, long scc, int sct, const float* eps, float* ws, void* stream);
/* The forward pass opens by re-packing every weight tensor into the plan's LDS-image order (ONE launch; the parameters change with
 * every optimizer step, solver.py:93).  A training loop moves that launch behind its optimizer step instead:
 *     avc_clip_adam_step(...); avc_plan_pack_weights(plan, params, ws, stream);          // end of step n
 *     avc_forward_ex(plan, params, ..., ws, AVC_FWD_WEIGHTS_PACKED, stream);             // step n + 1 opens with its first conv
 * AVC_FWD_WEIGHTS_PACKED is a promise that `params` has not changed since the last avc_plan_pack_weights into THIS workspace. */
#define AVC_FWD_WEIGHTS_PACKED 1
int avc_plan_pack_weights(const avc_plan* p, const float* params, float* ws, void* stream);
int avc_forward_ex(const avc_plan* p, const float* params, const float* x, long sxb, long sxc, int sxt,
                   const float* x_cond, long scb, long scc, int sct, const float* eps, float* ws, int flags, void* stream);

/* ---- ragged inference: B (source, target) pairs of DIFFERENT lengths in ONE launch set (the batched generalisation of
 * Inferencer.inference_one_utterance, inference.py:54-70; the reference converts one utterance per call).  Nothing is padded --
 * reflect padding, ceil-mode pooling and the InstanceNorm statistics all see each utterance's true length -- so result b equals
 * AE.inference(x_b, x_cond_b) (model.py:387-391).  T[b] / T_cond[b]: frames of source / target utterance b (host arrays).
 * x, x_cond: the utterances back to back as rows of frames, [sum T][M] fp32 (mel bins contiguous: the [T, M] arrays the
 * reference's utt_make_frames views).  Result: ws["dec"] holds the converted utterances back to back, utterance b as a
 * [M][out_len[b]] block (frames contiguous) at float offset out_off[b]; out_len[b] = 8 ceil(T[b] / 8) for the stock config. */
int avc_plan_create_ragged(const avc_model_cfg* cfg, int B, const int* T, const int* T_cond, const avc_tuning* tuning, avc_plan** out);
int avc_plan_ragged_out(const avc_plan* p, int* out_len, long* out_off);
int avc_forward_ragged(const avc_plan* p, const float* params, const float* x, const float* x_cond, float* ws, void* stream);
/* RAGGED PART PLANS (enrol a speaker once, convert from the embedding): avc_plan_create_ragged is avc_plan_create_ragged_ex with
 * flags = 0.  At most ONE of the two flags below; any other bit is refused.  Either plan packs only the weight images of the networks it
 * runs and allocates only their buffers and tables (avc_plan_workspace_floats is smaller than the whole ragged plan's), takes the full
 * flat parameter buffer, honours avc_plan_set_compute_dtype as a whole ragged plan does, and checks the reflect-pad rule for the
 * networks it runs only.  A branch runs the SAME kernel instances as in the whole ragged plan over the same lengths (the launch choice
 * is a function of the layer and of its own level tables only): in fp32 the results are bit-identical to the whole plan's.
 *  - AVC_PLAN_SPEAKER_ONLY: only the speaker encoder runs, over T_cond[0..B) (T is ignored and may be NULL).
 *    avc_forward_ragged(p, params, NULL, x_cond, ws, stream) leaves ws["emb"] [B, c_cond] fp32 contiguous; x_cond must not be NULL.
 *    One branch, one stream: every kernel goes to the caller's stream.  avc_plan_ragged_out is refused (there is no "dec").
 *  - AVC_PLAN_EMB_INPUT: the speaker encoder does not run (T_cond is ignored and may be NULL); the content encoder and the decoder run
 *    through avc_forward_ragged_emb, with the caller's embeddings in place of the speaker encoder's: emb is [B, c_cond] fp32 on the
 *    device, read in place with non-negative element strides (seb, sec) as avc_decoder_forward reads its emb.  seb = 0 is legal: ONE
 *    embedding for all B utterances.  Results are where a whole ragged plan leaves them (avc_plan_ragged_out, ws["dec"], ws["muls"]).
 *    avc_forward_ragged is refused on such a plan, avc_forward_ragged_emb on every other plan. */
#define AVC_PLAN_EMB_INPUT 512
int avc_plan_create_ragged_ex(const avc_model_cfg* cfg, int B, const int* T, const int* T_cond, int flags, const avc_tuning* tuning,
                              avc_plan** out);
int avc_forward_ragged_emb(const avc_plan* p, const float* params, const float* x, const float* emb, long seb, long sec, float* ws,
                           void* stream);
/* RAGGED FAN-OUT (encode each source once, decode it in many voices).  The plans above have ONE sample count for all three networks;
 * here the decoder has its own: S sources of T[s] frames, N outputs, output j is source src_of[j] (0 <= src_of[j] < S, any order, repeats
 * and unused sources legal) decoded with row j of the caller's embeddings.  The speaker encoder never runs (enrol first); forward only.
 * avc_plan_create_ragged / _ex are what they were and keep refusing the flags below.  `flags` takes three values, every other bit is
 * refused with -1:
 *  - 0: the content encoder runs over the S sources, the decoder over the N outputs, through avc_forward_ragged_emb(p, params, x, emb,
 *    seb, sec, ws, stream): x is [sum_s T[s]][M], each source ONCE; emb is [N, c_cond] under the stride rules of AVC_PLAN_EMB_INPUT
 *    (seb = 0: one voice for all outputs).  avc_plan_ragged_out reports N lengths and offsets.  The decoder's voice-independent first
 *    stage (in_conv + InstanceNorm + activation) runs once per SOURCE; its first block reads every output's source block through a
 *    mapped length / offset table.  Output j is bit-identical to output j of an AVC_PLAN_EMB_INPUT plan over the N expanded sources
 *    x[src_of[j]] (a column tile is 64 frames of one sample, the chunk depth of a ragged plan does not depend on its tile counts, the
 *    row kernels work row by row), in fp32 and with avc_plan_set_compute_dtype(1).
 *  - AVC_PLAN_CONTENT_ONLY: the content encoder alone; N must be 0 and src_of NULL.  avc_forward_ragged(p, params, x, NULL, ws, stream)
 *    leaves ws["muls"]; avc_plan_ragged_out is refused with -8.
 *  - AVC_PLAN_DECODER_ONLY: the decoder alone, from the caller's latents; T[s] are then the LATENT lengths Tz[s].  It runs through
 *    avc_decoder_forward_ragged: z holds the S latent blocks back to back, block s is [zc][Tz[s]] fp32 (frames contiguous) at float
 *    offset zc * offz[s] (offz = prefix sums of Tz), and its first c_in channel rows are read in place.  zc = 2 c_out takes the
 *    ws["muls"] region of a content plan over the same sources as it is (a pointer into ANOTHER workspace is fine), zc = c_in takes
 *    mu-only blocks; zc < c_in is refused with -1.  emb, seb, sec as above.
 * avc_plan_flags reports INFERENCE | RAGGED | EMB_INPUT for the first and the third kind, plus the part flag where there is one, plus
 * AVC_PLAN_FANOUT on all three.  Each forward entry point refuses the wrong kind of plan with -8 and avc_last_error names the call to
 * use.  A network that does not run gets no weight image, no pack-table row, no tables and no buffers; the reflect-pad rule (-6) is
 * checked for the networks that run only (a decoder plan: on Tz of the sources that have an output).  avc_plan_set_compute_dtype
 * works on all three kinds.  One branch: every kernel goes to the caller's stream, no fork, no join.
 *   avc_plan_ragged_latents (every ragged plan with a content encoder, the plans of avc_plan_create_ragged / _ex included; -8 on
 * speaker-only and decoder-only plans): per SOURCE s its latent length len[s] (ceil(T[s] / 8) for the stock config) and the float
 * offset off[s] of its [2 c_out][len[s]] block in the workspace (ws["muls"]; mu rows first, then log_sigma). */
#define AVC_PLAN_FANOUT 1024   /* set by avc_plan_create_ragged_fanout (reported by avc_plan_flags); refused by every other creator */
int avc_plan_create_ragged_fanout(const avc_model_cfg* cfg, int S, const int* T, int N, const int* src_of, int flags,
                                  const avc_tuning* tuning, avc_plan** out);
int avc_plan_ragged_latents(const avc_plan* p, int* len, long* off);
int avc_decoder_forward_ragged(const avc_plan* p, const float* params, const float* z, int zc, const float* emb, long seb, long sec,
                               float* ws, void* stream);
/* INPUT GRADIENTS THROUGH RAGGED ENROLMENT: avc_plan_create_ragged_ex(AVC_PLAN_SPEAKER_ONLY | AVC_PLAN_INPUT_GRADS).  The flag is
 * refused with AVC_PLAN_EMB_INPUT and on a whole ragged plan (flags without a part flag): through this creator only the ragged SPEAKER
 * ENCODER has a backward pass (the content encoder's: avc_plan_create_ragged_content_grads below).  Without the flag a speaker-only plan is what it was (pack table, workspace, launches).  With it the plan also packs the
 * input-gradient weight images (transposed, tap-flipped) of the speaker encoder's convs, of its conv bank, of the in_conv's M
 * pass-through rows and of the dense stack, and allocates the gradient temporaries and ws["d_x_cond"]; its forward pass is bit-identical
 * to the unflagged plan's.
 *   avc_backward_ragged follows an avc_forward_ragged on the SAME plan, params, x_cond and workspace (the forward leaves the activations,
 * the weight images and the level tables there).  d_emb: d(loss)/d(emb) [B, c_cond] fp32 on the device, read in place with non-negative
 * element strides (seb, sec) that span less than 2^31 elements, as avc_forward_ragged_emb reads emb; seb = 0 (an expanded row) is legal.
 * params and x_cond must not be NULL but are RESERVED: the pass reads the weight images and activations the forward left in the
 * workspace, not the parameter buffer or the input (pass what the forward got).  Result: ws["d_x_cond"] =
 * d(loss)/d(x_cond) in x_cond's own layout, [sum T_cond][M] fp32 (utterance b = rows off[b] .. off[b] + T_cond[b]).  fp32 only (a plan
 * whose compute dtype was set to bf16 is refused with -8: `bf16r` is a forward-only rounding model).  Parameters are frozen: no
 * parameter gradient is computed, no weight-gradient launch is made.  No atomics and a fixed summation order (the nb + 1 terms of
 * d(x_cond) are summed through the residual join of consecutive launches): two passes give identical bits.  Every kernel goes to the
 * caller's stream; the call only enqueues (no allocation, no copy from the host, no synchronisation).  Refused with -8 on any plan
 * that was not created with both flags. */
int avc_backward_ragged(const avc_plan* p, const float* params, const float* x_cond, const float* d_emb, long seb, long sec, float* ws,
                        void* stream);
/* PARAMETER GRADIENTS OF THE RAGGED SPEAKER ENCODER: avc_plan_create_ragged_speaker_grads(cfg, B, T_cond, tuning, out) creates the flagged
 * speaker plan above (AVC_PLAN_SPEAKER_ONLY | AVC_PLAN_INPUT_GRADS) with, on top of it, the weight gradient's K-chunk tables (32 frames of ONE
 * utterance per chunk, next to the level tables), one d(pre-activation) row set per dense layer and the split-K slots of every layer that is
 * split.  avc_plan_flags additionally reports AVC_PLAN_PART_GRADS.  Its forward (avc_forward_ragged) launches the same kernel instances on the
 * same operands as the unflagged speaker plan: ws["emb"] is bit-identical.  avc_backward_ragged works on it as on the flagged plan (the frozen
 * pass: no weight-gradient launch, ws["d_x_cond"] bit-identical to that plan's).  The existing creators keep refusing what they refused.
 *   avc_backward_ragged_params follows an avc_forward_ragged on the SAME plan, params, x_cond and workspace; d_emb, seb, sec, params and x_cond
 * as for avc_backward_ragged.  It is that pass plus d(loss)/d(parameters): behind each phase that produces a layer's output gradient, and
 * before the ping-pong gradient rows are overwritten, one launch of the ragged weight-gradient kernel (csrc/conv_wgrad_ragged.hip; fp32 MFMA
 * products): the 2 nd + 1 Linears of the dense stack together (their [c_h][B] rows are one sample of B frames), the two convs of every block
 * together, the in_conv and all bank members together; then ONE reduce launch sums the split layers' slots in slot order: n + 3 launches on
 * top of the frozen pass (9 for the stock 6 blocks).  `grads` is the full flat gradient buffer (the layout of params): the pass OVERWRITES
 * every tensor of the speaker encoder's range (avc_plan_param_range(AVC_GRADS_SPEAKER); weights and biases) and touches nothing else.
 * ws["d_x_cond"] is written as by avc_backward_ragged, bit for bit.  No atomics, a fixed summation order: two passes give identical bits.
 * Every kernel goes to the caller's stream; the call only enqueues (no allocation, no copy from the host, no synchronisation).  fp32 only
 * (-8 when the plan's compute dtype is bf16); -8 with a message naming the creator on any other plan; -1 on a null argument. */
int avc_plan_create_ragged_speaker_grads(const avc_model_cfg* cfg, int B, const int* T_cond, const avc_tuning* tuning, avc_plan** out);
int avc_backward_ragged_params(const avc_plan* p, const float* params, const float* x_cond, const float* d_emb, long seb, long sec,
                               float* grads, float* ws, void* stream);
/* INPUT GRADIENTS THROUGH THE RAGGED CONTENT ENCODER:avc_plan_create_ragged_content_grads(cfg, S, T, tuning, out) creates the content
 * encoder alone over S sources of T[s] frames -- the AVC_PLAN_CONTENT_ONLY plan of avc_plan_create_ragged_fanout -- with a backward pass
 * with respect to its input.  avc_plan_flags reports what that plan reports plus AVC_PLAN_INPUT_GRADS; avc_plan_ragged_latents works; the
 * reflect-pad rule is the forward plan's (-6).  Its forward runs through avc_forward_ragged(p, params, x, NULL, ws, stream) and launches
 * the same kernel instances on the same operands as the plan without a backward pass: ws["muls"] is bit-identical.  On top of that plan
 * it packs (in the plan's one pack launch) the input-gradient weight images (transposed, tap-flipped) of the blocks' convs, the heads, the
 * in_conv, the conv bank and the in_conv's M pass-through rows, its InstanceNorm launches store the mean / rstd of every row, and the
 * workspace holds d(cat), ws["d_x"] and two ping-pong pairs of gradient rows.  The existing creators keep refusing AVC_PLAN_INPUT_GRADS
 * wherever they did, and avc_backward_ragged keeps refusing every plan that is not a flagged speaker plan, this one included.
 *   avc_content_backward_ragged follows an avc_forward_ragged on the SAME plan, params, x and workspace.  d_muls: d(loss)/d(mu | log_sigma),
 * fp32, contiguous, in the layout of ws["muls"]: block s is [2 c_out][Tz_s] at float offset 2 c_out * offz[s] (avc_plan_ragged_latents),
 * mu rows first, then log_sigma rows.  params and x must not be NULL but are RESERVED (the pass reads the weight images, pre-norm rows and
 * statistics the forward left in the workspace).  Result: ws["d_x"] = d(loss)/d(x) in x's own layout, [sum T][M] fp32.  Launches, in
 * order: the heads' 1x1 input gradient; per block from last to first InstanceNorm backward of y2 (one wavefront per row at the row's own
 * length, the ReLU decision recomputed from the SAVED statistics: the forward's, bit for bit), conv2's input gradient, InstanceNorm
 * backward of y1, conv1's input gradient with the pool / identity adjoint of the residual path in its epilogue join; InstanceNorm backward
 * of the in_conv's rows; the in_conv's input gradient masked by cat > 0; the nb + 1 terms of d(x) summed through the residual join of
 * consecutive launches.  fp32 only (-8 when the plan's compute dtype is bf16), parameters frozen, no weight gradients, no atomics, a fixed
 * summation order: two passes give identical bits.  Every kernel goes to the caller's stream; the call only enqueues.  -8 on any other
 * plan, -1 on a null argument.  Further named buffers of such a plan (avc_plan_buffer): "enc_cat" (the concat buffer), "enc_y0",
 * "enc_y1_<l>", "enc_y2_<l>" (the pre-norm rows, packed [c_h][T_s] blocks) and "enc_st0", "enc_st1_<l>", "enc_st2_<l>" (their statistics:
 * mean[S * c_h] then rstd[S * c_h], row s * c_h + c). */
int avc_plan_create_ragged_content_grads(const avc_model_cfg* cfg, int S, const int* T, const avc_tuning* tuning, avc_plan** out);
int avc_content_backward_ragged(const avc_plan* p, const float* params, const float* x, const float* d_muls, float* ws, void* stream);
/* INPUT GRADIENTS THROUGH THE RAGGED DECODER: avc_plan_create_ragged_decoder_grads(cfg, N, Tz, tuning, out) creates the decoder alone over
 * N latents of Tz[j] frames, output j from latent j, with a backward pass with respect to its two inputs z and emb.  avc_plan_flags reports
 * AVC_PLAN_RAGGED | AVC_PLAN_EMB_INPUT | AVC_PLAN_DECODER_ONLY | AVC_PLAN_INPUT_GRADS (no AVC_PLAN_FANOUT: the map is the identity; callers
 * that decode one latent in several voices index the latents themselves and sum the gradients); avc_plan_ragged_out works; the reflect-pad
 * rule is the forward plan's (-6).  Its forward runs through avc_decoder_forward_ragged and launches the same kernel instances on the same
 * operands as the decoder-only plan of avc_plan_create_ragged_fanout with the identity map: ws["dec"] is bit-identical.  On top of that plan
 * it packs (in the plan's one pack launch) the input-gradient weight images of out_conv, both convs of every block, in_conv and the stacked
 * AdaIN affine Linears, its InstanceNorm launches store the mean / rstd of every row, and the workspace holds ws["d_cond"], two ping-pong
 * pairs of gradient rows, ws["d_z"] and ws["d_emb"].  Plans created any other way keep their pack table, workspace and launches.
 *   avc_decoder_backward_ragged follows an avc_decoder_forward_ragged on the SAME plan, params, z, emb and workspace.  d_dec:
 * d(loss)/d(dec), fp32, contiguous, packed [M][T''_j] blocks in the order and at the relative offsets avc_plan_ragged_out reports.  z, zc,
 * emb, seb, sec: the forward's (checked like the forward's; seb = 0 is legal; RESERVED otherwise: the pass reads the weight images, pre-norm
 * rows, statistics and ws["cond"] the forward left in the workspace).  Results: ws["d_z"], blocks [c_in][Tz_s] at float offset c_in * offz[s]
 * (offz = prefix sums of Tz), and ws["d_emb"], dense row-major [N][c_cond] whatever seb was (a caller that expanded one voice sums the rows).
 * Launches, in order: out_conv's input gradient; per block from last to first AdaIN backward of y2 (one wavefront per row at the row's own
 * length, the activation decision recomputed from the SAVED statistics and ws["cond"]: the forward's, bit for bit; lane 0 stores the row's
 * d(beta), d(gamma) into ws["d_cond"]; behind an upsampling block the rows are stored as the conv's own [c_h up][T_l] output rows), conv2's
 * input gradient, AdaIN backward of y1, conv1's input gradient with the nearest-upsampling / identity adjoint of the residual path in its
 * epilogue join; InstanceNorm backward of the in_conv's rows; the in_conv's input gradient into ws["d_z"]; d(emb) = W_affine^T d(cond), one
 * uniform input-gradient launch over N columns storing row-major: 1 + 4 n + 3 launches.  One pass writes every element of ws["d_cond"]
 * exactly once: nothing is zeroed.  fp32 only, parameters frozen, no weight gradients, no atomics, a fixed summation order: two passes give
 * identical bits.  Every kernel goes to the caller's stream; the calls allocate nothing and synchronise nothing.  -8 with a message naming
 * the creator on a plan without AVC_PLAN_INPUT_GRADS, on a fan-out plan and when the plan's compute dtype is bf16; -1 on a null argument.
 * Further named buffers of such a plan (avc_plan_buffer): "dec_y0", "dec_y1_<l>", "dec_y2_<l>" (pre-norm rows, packed [c_h][T] blocks at the
 * level of the row), "dec_a1_<l>" (the first conv's activations), "dec_st0", "dec_st1_<l>", "dec_st2_<l>" (mean[N * c_h] then rstd[N * c_h],
 * row j * c_h + c) and "cond" / "d_cond" ([N][2 n 2 c_h]: stage k = 2 l (+ 1 for the second conv) holds beta at 2 k c_h, gamma at (2 k + 1) c_h). */
int avc_plan_create_ragged_decoder_grads(const avc_model_cfg* cfg, int N, const int* Tz, const avc_tuning* tuning, avc_plan** out);
int avc_decoder_backward_ragged(const avc_plan* p, const float* params, const float* z, int zc, const float* emb, long seb, long sec,
                                const float* d_dec, float* ws, void* stream);
/* PARAMETER GRADIENTS OF THE RAGGED CONTENT ENCODER AND DECODER: avc_plan_create_ragged_content_param_grads(cfg, S, T, tuning, out) and
 * avc_plan_create_ragged_decoder_param_grads(cfg, N, Tz, tuning, out) create the plans of avc_plan_create_ragged_content_grads /
 * _decoder_grads with, on top of them, the weight gradient's K-chunk tables on every level, ONE more set of gradient rows (so that both
 * output gradients of a block are live at once and share one weight-gradient launch) and the split-K slots of every layer that is split.
 * avc_plan_flags additionally reports AVC_PLAN_PART_GRADS.  The forward passes (avc_forward_ragged / avc_decoder_forward_ragged) launch the
 * same kernel instances on the same operands as those plans: ws["muls"] / ws["dec"] are bit-identical.  avc_content_backward_ragged /
 * avc_decoder_backward_ragged work on the new plans as on the old (the frozen passes: no weight-gradient launch; ws["d_x"], ws["d_z"],
 * ws["d_emb"] bit-identical).  The existing creators keep refusing what they refused; the frozen plans' workspaces are what they were.
 *   avc_content_backward_ragged_params follows an avc_forward_ragged on the SAME plan, params, x and workspace; d_muls as for
 * avc_content_backward_ragged.  It is that pass plus d(loss)/d(parameters) from the ragged weight-gradient kernel
 * (csrc/conv_wgrad_ragged.hip): per block ONE launch with conv2's and conv1's jobs (the two heads ride in the first block's launch: their dy
 * is the caller's d_muls), one launch with the in_conv and all bank members, then ONE reduce launch: n + 2 launches on top of the frozen
 * pass (8 for the stock 6 blocks).  `grads` is the full flat gradient buffer: the pass OVERWRITES every tensor of the content encoder's range
 * (avc_plan_param_range(AVC_GRADS_CONTENT); weights and biases -- the bias of a conv that feeds an InstanceNorm gets its mathematically zero
 * gradient as the rounding residue of its row sums) and touches nothing else.
 *   avc_decoder_backward_ragged_params follows an avc_decoder_forward_ragged on the SAME plan, params, z, zc, emb, seb, sec and workspace;
 * here z and emb are READ (the in_conv's weight gradient reads the latent blocks in place, the 2 n AdaIN affine Linears' read emb through
 * (seb, sec); seb = 0 is legal): they must be the forward's.  The jobs: out_conv (dy = the caller's d_dec) and the last block's two convs in
 * one launch, one launch per other block, then the in_conv and the 2 n affine Linears (STRIDED jobs: dy = the layer's [N][2 c_h] slice of
 * frame-major ws["d_cond"]) in one launch, then ONE reduce launch: n + 2 launches on top of the frozen pass.  The pass OVERWRITES every
 * tensor of avc_plan_param_range(AVC_GRADS_DECODER) and touches nothing else; ws["d_z"] and ws["d_emb"] are the frozen pass's, bit for bit.
 *   Both: no atomics, a fixed summation order (two passes give identical bits); every kernel goes to the caller's stream; the call only
 * enqueues.  fp32 only (-8 when the plan's compute dtype is bf16); -8 with a message naming the creator on any other plan; -1 on a null
 * argument. */
int avc_plan_create_ragged_content_param_grads(const avc_model_cfg* cfg, int S, const int* T, const avc_tuning* tuning, avc_plan** out);
int avc_content_backward_ragged_params(const avc_plan* p, const float* params, const float* x, const float* d_muls, float* grads, float* ws,
                                       void* stream);
int avc_plan_create_ragged_decoder_param_grads(const avc_model_cfg* cfg, int N, const int* Tz, const avc_tuning* tuning, avc_plan** out);
int avc_decoder_backward_ragged_params(const avc_plan* p, const float* params, const float* z, int zc, const float* emb, long seb, long sec,
                                       const float* d_dec, float* grads, float* ws, void* stream);

/* L1 + KL losses of solver.py:84-86 -> ws["losses"] = {loss_rec, loss_kl}; writes
 * d(lambda_rec*loss_rec)/d(dec) into ws["d_dec"] for avc_backward. */
int avc_loss(const avc_plan* p, const float* x, long sxb, long sxc, int sxt, float lambda_rec, float* ws, void* stream);

/* backward of avc_forward (autograd of model.py:380-385).  d_dec [B,M,T'] (NULL = use
 * ws["d_dec"] from avc_loss), d_muls_up [B,2*c_out,Tb] and d_emb_up [B,c_cond] are
 * upstream gradients (may be NULL); lambda_kl adds the KL term of solver.py:86-88
 * analytically (0 = none).  Writes every parameter gradient into the flat `grads`
 * buffer (same layout as params). */
int avc_backward(const avc_plan* p, const float* params, const float* x, long sxb, long sxc, int sxt,
                 const float* x_cond, long scb, long scc, int sct, const float* eps, const float* d_dec,
                 const float* d_muls_up, const float* d_emb_up, float lambda_kl, float* grads, float* ws, void* stream);

/* ---- decoder part plans (AVC_PLAN_DECODER_ONLY): Decoder.forward(z, cond) (model.py:347-371) and its autograd.
 * z: [B, c_in, Tb] with any element strides (szb, szc, szt); emb: [B, c_cond] with any strides (seb, sec).  Both are read in
 * place (fp32 plans: the in_conv and its weight gradient read z, the AdaIN affine GEMM and its weight gradient read emb; AVC_PLAN_BF16S
 * plans first convert z to bf16 pairs).  Enqueue only: no allocation, no synchronisation, graph-capture safe.
 * avc_decoder_forward leaves ws["dec"] [B, M, Tb * prod(upsample)]; flags: AVC_FWD_WEIGHTS_PACKED as for avc_forward_ex.
 * avc_decoder_backward (AVC_PLAN_PART_GRADS plans, after avc_decoder_forward with the same z / emb / params): d_dec [B, M, Tout]
 * contiguous (NULL = ws["d_dec"]); writes the decoder's range of `grads` and leaves ws["d_z"] ([B, c_in, Tb] fp32 contiguous) and
 * ws["d_emb"] ([B, c_cond] fp32 row-major): the gradients with respect to the caller's z and emb (no reparameterisation step runs). */
int avc_decoder_forward(const avc_plan* p, const float* params, const float* z, long szb, long szc, int szt, const float* emb, long seb,
                        long sec, float* ws, int flags, void* stream);
int avc_decoder_backward(const avc_plan* p, const float* params, const float* z, long szb, long szc, int szt, const float* emb, long seb,
                         long sec, const float* d_dec, float* grads, float* ws, void* stream);

/* ---- bf16 PAIR storage (compute_dtype "bf16", BASELINE configs[2]): an activation tensor [B, C, T] is a DWORD tensor [B][C/2][T],
 * dword (b, p, t) = bf16(channel 2p) in the low half, bf16(channel 2p + 1) in the high half; statistics and accumulation stay fp32.
 * Op-level conv launches select it with avc_set_tuning("op_compute_dtype", 3) (pair tensors in and out; strides in dwords; 4 = pair
 * operands with fp32 outputs, as the heads and the decoder's last conv run); avc_pack_weight then emits bf16 pair weight images.
 * InstanceNorm / AdaIN rows (reference: model.py:296,341,77-83 and autograd): planar != 0 reads y (writes dy) as natural bf16
 * [B][C][T] rows -- the layout a pixel-shuffling conv (model.py:52-59) leaves its output in. */
int avc_instnorm_fwd_pairs(const void* y, int B, int C, int T, const float* cond, long cond_sb, int cond_off, int relu, const void* res, int res_mode,
                           int Tres, int planar, void* out, float* mean, float* rstd, void* stream);
int avc_instnorm_bwd_pairs(const void* g, const void* y, const float* mean, const float* rstd, int B, int C, int T, const float* cond, long cond_sb,
                           int cond_off, int relu, int planar, void* dy, float* dcond, long dcond_sb, int dcond_off, void* stream);
int avc_to_pairs(const float* x, long sxb, long sxc, long sxt, int B, int C, int T, void* dst, void* stream);

/* clip_grad_norm_(max_norm) + torch.optim.Adam(amsgrad, coupled L2) of solver.py:75-77,
 * :91-93 on flat buffers.  step is 1-based.  grad_prescale = 1/world_size when g holds an
 * all-reduced SUM.  ws: avc_clip_adam_ws_floats(n) floats.  gnorm_out: device float or NULL. */
long avc_clip_adam_ws_floats(long n);
int avc_clip_adam_step(float* p, float* g, float* m, float* v, float* vmax, long n, int step, float lr, float beta1,
                       float beta2, float eps, float weight_decay, int amsgrad, float max_norm, float grad_prescale,
                       int write_clipped, float* ws, float* gnorm_out, void* stream);

/* Edits ONE field (by name, as in the struct above; also "compute" = op_compute_dtype) of the CALLING THREAD's op-level tuning:
 * it affects only the op-level entry points at the end of this header when called from the same thread (micro-benchmark
 * scripts, kernel tests), never a plan.  Returns -1 for an unknown name.  avc_get_op_tuning copies the current value. */
int avc_set_tuning(const char* name, int value);
void avc_get_op_tuning(avc_tuning* out);

/* ---- device-side segment feed (replaces PickleDataset.__getitem__ + CollateFn, data_utils.py:10-22,51-54,
 * for an HBM-resident corpus): out[b, m, t] = corpus[starts[b] + t, m], corpus = [n_rows, M] fp32 (mel bins
 * contiguous), starts = B device int64 row indices, out = [B, M, T] contiguous. */
int avc_gather_segments(const float* corpus, long n_rows, int M, const long* starts, int B, int T, float* out,
                        void* stream);

/* ---- mel <-> waveform DSP (replaces preprocess/tacotron/utils.py:27-155, there librosa on the CPU)
 * A complex spectrogram is [2F][T] fp32 (row 2f = Re, 2f+1 = Im of bin f, F = n_fft/2 + 1, T contiguous); magnitudes /
 * mels are [C][T]; the normalised features the pickles and the model use are [T][C] (utils.py:84-85).
 * The transforms are GEMMs against DFT bases that carry the centre-padded periodic Hann window (built once per
 * (n_fft, win_length) by avc_dsp_make_basis into caller memory of avc_dsp_basis_floats floats; dense_scratch:
 * avc_dsp_basis_scratch_floats floats, free afterwards).  Nothing here allocates or synchronises. */
int avc_dsp_num_frames(long L, int hop_length);                      /* librosa.stft(center=True): 1 + L / hop */
long avc_dsp_basis_floats(int n_fft, int win_length, int inverse);
long avc_dsp_basis_scratch_floats(int n_fft, int win_length);
int avc_dsp_make_basis(int n_fft, int hop_length, int win_length, int inverse, float* dense_scratch, float* packed, void* stream);
/* librosa.stft(y, n_fft, hop_length, win_length) (utils.py:63-66,141): reflect padding of n_fft/2, T = 1 + L/hop frames.
 * frames_ws: win_length * T floats.  -6 when L <= n_fft/2 (the reference's call raises there). */
int avc_dsp_stft(const float* y, long L, int n_fft, int hop_length, int win_length, const float* basis_fwd, float* frames_ws,
                 float* spec, void* stream);
/* librosa.istft(spec, hop_length, win_length, window="hann") (utils.py:150-154): y has hop * (T - 1) samples. */
int avc_dsp_istft(const float* spec, int T, int n_fft, int hop_length, int win_length, const float* basis_inv, float* tf_ws, float* y,
                  void* stream);
/* griffin_lim (utils.py:136-147) on magnitudes S [F][T]: n_iter x (istft, stft, phase projection) + the final istft. */
long avc_dsp_griffin_lim_ws_floats(int T, int n_fft, int hop_length, int win_length);
int avc_dsp_griffin_lim(const float* S, int T, int n_fft, int hop_length, int win_length, int n_iter, const float* basis_fwd,
                        const float* basis_inv, float* ws, float* y, void* stream);
/* B equally long utterances at once: their frames are the columns of ONE GEMM per transform (a lone 400-frame utterance is
 * 133-238 workgroups).  y: [B][L] signals -> spec [2F][B T] with utterance b in columns b T .. b T + T - 1; S likewise [F][B T];
 * waveforms [B][hop (T - 1)].  Workspaces: the single-utterance sizes with T replaced by B T. */
int avc_dsp_stft_batch(const float* y, long L, int B, int n_fft, int hop_length, int win_length, const float* basis_fwd, float* frames_ws,
                       float* spec, void* stream);
int avc_dsp_istft_batch(const float* spec, int B, int T, int n_fft, int hop_length, int win_length, const float* basis_inv, float* tf_ws,
                        float* y, void* stream);
int avc_dsp_griffin_lim_batch(const float* S, int B, int T, int n_fft, int hop_length, int win_length, int n_iter, const float* basis_fwd,
                              const float* basis_inv, float* ws, float* y, void* stream);
/* ... and of DIFFERENT lengths: toff = B + 1 device ints (first frame of every utterance, toff[B] = Ttot), toff_host = the same
 * offsets in host memory (validated here: -1 unless monotone from 0 to Ttot, -6 unless every utterance has hop (T_b - 1) > n_fft / 2,
 * the reflect padding of its STFT; the kernels index through the device copy unchecked); S is [F][Ttot]; the waveforms come back to
 * back, utterance b (hop (T_b - 1) samples) at sample hop (toff[b] - b).  ws: avc_dsp_griffin_lim_ws_floats(Ttot, ...). */
int avc_dsp_griffin_lim_ragged(const float* S, const int* toff, const int* toff_host, int B, int Ttot, int n_fft, int hop_length, int win_length,
                               int n_iter, const float* basis_fwd, const float* basis_inv, float* ws, float* y, void* stream);
int avc_dsp_magnitude(const float* spec, int n_fft, int T, float* mag, void* stream);                                   /* utils.py:69 */
/* out[t][c] = clip((20 log10(max(1e-5, in[c][t])) - ref_db + max_db) / max_db, 1e-8, 1)   (utils.py:76-85) */
int avc_dsp_db_normalize(const float* in, int C, int T, float ref_db, float max_db, float* out, void* stream);
/* out[c][t] = 10 ^ (0.05 (clip(in[t][c], 0, 1) max_db - max_db + ref_db))                 (utils.py:92-98) */
int avc_dsp_denormalize_amp(const float* in, int C, int T, float ref_db, float max_db, float* out, void* stream);
int avc_dsp_preemphasis(const float* y, long L, float a, float* out, void* stream);        /* utils.py:60 (out != y) */
int avc_dsp_deemphasis(const float* x, long L, float a, float* out, void* stream);         /* utils.py:104 lfilter([1], [1, -a]) */
/* mean square of the frames of librosa.effects.trim (utils.py:57,107): out[1 + (L - frame_length % 2) / hop] */
int avc_dsp_frame_power(const float* y, long L, int frame_length, int hop_length, float* out, void* stream);
/* The two audio edges for B utterances of DIFFERENT lengths in one launch each.  The waveforms lie back to back in one buffer:
 * utterance b is samples woff[b] .. woff[b+1] (woff: B + 1 device int64 from 0, every utterance at least one sample).  Every table
 * comes twice, as for avc_dsp_griffin_lim_ragged: the device copy the kernels index through unchecked and the HOST copy validated here;
 * a refused call launches nothing.  Each result is bit-equal to the single-utterance entry point called per utterance.
 * frame_power_ragged: utterance b's powers at out[poff[b] .. poff[b+1]) (poff: B + 1 int32 from 0, poff[b+1] - poff[b] = the frame count of
 *   avc_dsp_frame_power; -1 otherwise); -6 when an utterance has L_b <= frame_length / 2.
 * frames_ragged_preemph: avc_dsp_preemphasis fused into the framing of avc_dsp_stft.  Utterance b is the sub-run [s_b, e_b) of its
 *   samples, (s_b, e_b) = bounds[2b], bounds[2b+1] (2B int64: the trim indices, or 0 and L_b); frames is [win_length][Ttot] with its
 *   T_b = 1 + (e_b - s_b) / hop frames in columns toff[b] .. toff[b+1] - 1 (toff: B + 1 int32 from 0; -1 when it disagrees with the bounds);
 *   -6 when an utterance has e_b - s_b <= n_fft / 2.  spec = avc_conv1d_fwd(basis_fwd, frames) as inside avc_dsp_stft.
 * deemphasis_ragged: avc_dsp_deemphasis on every utterance, one workgroup each (x == out allowed). */
int avc_dsp_frame_power_ragged(const float* y, const long* woff, const long* woff_host, const int* poff, const int* poff_host, int B,
                               int frame_length, int hop_length, float* out, void* stream);
int avc_dsp_frames_ragged_preemph(const float* y, const long* woff, const long* woff_host, const int* toff, const int* toff_host, const long* bounds,
                                  const long* bounds_host, int B, int n_fft, int hop_length, int win_length, float a, float* frames, void* stream);
int avc_dsp_deemphasis_ragged(const float* x, const long* woff, const long* woff_host, int B, float a, float* out, void* stream);

/* ---- op-level entry points (one per kernel family and direction) -------- */
long avc_packed_weight_floats(int Cout, int Cin, int KS, int dgrad);
/* W[Cout][Cin][KS] (nn.Conv1d / nn.Linear state_dict layout; nsrc tensors stacked on Cout) -> LDS-image order of
 * csrc/conv_gemm.hip: [chunk][tap][8-channel unit][lane half h][row m][k-step u], channel = 8 unit + 2 u + h (16-byte fragments) */
int avc_pack_weight(const float* const* srcs, int nsrc, int rows_per_src, int Cout, int Cin, int KS, int dgrad,
                    float* dst, void* stream);
/* weight image of the split-bf16 conv kernel (csrc/conv_x3.hip; k = 5, reduction channels a multiple of 16: every operand as
 * three bf16 terms, six bf16 MFMAs per product block, fp32-level accuracy): pass it as `wp` / `wpd` together with tile = 97.
 * Whole-model plans created with AVC_PLAN_X3 (or tuning.conv_x3) use it for their k = 5 layers that fill the chip (opt-in; the
 * default engine multiplies in exact fp32). */
long avc_packed_weight_floats_x3(int Cout, int Cin, int KS, int dgrad);
int avc_pack_weight_x3(const float* w, int Cout, int Cin, int KS, int dgrad, float* dst, void* stream);
/* pad_layer (model.py:21-32): y = act(conv1d(reflect_pad(x), W) + b) (act: 0 none, 1 ReLU, 2 LeakyReLU(0.01)); ops = pixel_shuffle_1d factor of the store
 * (model.py:52-59); res/res_mode: y2 = y + resmap(res) (1 identity, 2 avg_pool1d(2, ceil_mode) model.py:248) */
int avc_conv1d_fwd(const float* x, long sxb, long sxc, int sxt, int B, int Cin, int Tin, const float* wp,
                   const float* bias, int Cout, int KS, int stride, int act, float* out, long ob, long oc, int ot,
                   int ops, const float* res, int res_mode, long rb, long rc, int rt, int Tres, float* out2, int tile,
                   void* stream);
/* input gradient incl. the adjoint of the reflect padding; res_mode 1 identity, 3 adjoint of avg-pool,
 * 4 adjoint of nearest-x2 upsample; dx2 = dx * (mask > 0) */
int avc_conv1d_dgrad(const float* dy, long syb, long syc, int syt, int yps, int B, int Cout, int Tdy, const float* wpd,
                     int Cin, int KS, int stride, int Tin, float* dx, long ob, long oc, int ot, const float* res,
                     int res_mode, long rb, long rc, int rt, int Tres, float* dx2, const float* mask, int tile,
                     void* stream);
long avc_conv1d_wgrad_ws_floats(int B, int Cin, int Cout, int Tout, int KS);
int avc_conv1d_wgrad(const float* x, long sxb, long sxc, int sxt, const float* dy, long syb, long syc, int syt, int yps,
                     int B, int Cin, int Cout, int Tin, int Tout, int KS, int stride, float* dW, float* db, float* ws,
                     void* stream);
/* ... over B samples of DIFFERENT lengths T[b] (host array), each with its own reflect padding; Tout_b = ceil(T[b] / stride), stride 1 or 2,
 * KS 1..8.  x and dy are packed as the ragged plans pack activations: sample b of x is a [xC][T[b]] block (frames contiguous) at float
 * offset xC * sum(T[0..b)), of which the Cin channels from xc0 are read; dy likewise, [dyC][Tout_b] blocks, Cout channels from dyc0.  dW is
 * [Cout][Cin][KS] (the parameter layout), db [Cout] or NULL; both are OVERWRITTEN.  ws: avc_conv1d_wgrad_ragged_ws_floats floats (-1 for bad
 * arguments).  The call builds its length / offset / K-chunk tables itself and uploads them (a few KB) to the head of ws with ONE
 * hipMemcpyAsync from pageable host memory on `stream`: it may block the host until the copy is staged and is NOT graph-capture safe; it
 * allocates no device memory and does not synchronise the device.  fp32 MFMA products, no atomics, a fixed order: two calls give identical
 * bits.  -6 when a sample is not longer than its left pad (KS / 2), -1 for any other bad argument. */
long avc_conv1d_wgrad_ragged_ws_floats(int B, const int* T, int Cin, int Cout, int KS, int stride);
int avc_conv1d_wgrad_ragged(const float* x, int xC, int xc0, const float* dy, int dyC, int dyc0, int B, const int* T, int Cin, int Cout,
                            int KS, int stride, float* dW, float* db, float* ws, void* stream);
/* ... of a Linear over N rows read through element strides: dW[co][ci] = sum_n dy(n, co) x(n, ci), db[co] = sum_n dy(n, co) with
 * x(n, ci) = x[n sxn + ci sxc] and dy(n, co) = dy[n syn + co syc].  All strides >= 0 and spanning less than 2^31 elements; a row stride of 0
 * is legal (every row reads the same one: an expanded single voice).  ONE strided job of the same kernel, the N rows are its frames: the
 * staging loops run along whichever axis of each operand has stride 1 (coalesced loads either way), the chunks of 32 rows, the MFMA chain,
 * the split-K slots and the slot-order reduce are avc_conv1d_wgrad_ragged's -- with sxn = syn = 1, sxc = syc = N the result is bit-identical
 * to that call at B = 1, T = {N}, KS = 1.  dW [Cout][Cin] and db [Cout] (or NULL) are OVERWRITTEN.  ws: avc_linear_wgrad_strided_ws_floats
 * floats (-1 for bad arguments).  No table, no copy from the host: the call only enqueues.  Two calls give identical bits.  -1 for a bad
 * argument. */
long avc_linear_wgrad_strided_ws_floats(int N, int Cin, int Cout);
int avc_linear_wgrad_strided(const float* x, long sxn, long sxc, const float* dy, long syn, long syc, int N, int Cin, int Cout, float* dW,
                             float* db, float* ws, void* stream);
/* nn.InstanceNorm1d(affine=False) (model.py:296,341) [+ append_cond model.py:77-83] [+ ReLU] [+ residual:
 * 1 identity, 2 avg-pool(ceil), 5 nearest x2]; cond row b: beta = cond[b*cond_sb + cond_off + c], gamma = [.. + C + c] */
/* relu: 0 = no activation, 1 = ReLU, 2 = LeakyReLU(0.01) */
int avc_instnorm_fwd(const float* y, int B, int C, int T, const float* cond, long cond_sb, int cond_off, int relu,
                     const float* res, int res_mode, int Tres, float* out, float* mean, float* rstd, void* stream);
int avc_instnorm_bwd(const float* g, const float* y, const float* mean, const float* rstd, int B, int C, int T,
                     const float* cond, long cond_sb, int cond_off, int relu, float* dy, float* dcond, long dcond_sb,
                     int dcond_off, void* stream);
/* conv -> InstanceNorm -> [append_cond] -> act [-> + residual] of one block half (model.py:309-320 / :353-369), exact fp32:
 * y = conv1d(reflect_pad(x)) + bias, pixel-shuffled on store when ops == 2 (model.py:52-59); out / mean / rstd as avc_instnorm_fwd over the
 * rows of y.  y, out, res are contiguous [B][C][T] with C = Cout / ops, T = Tout * ops.  Where the conv's output rows are 16 / 32 / 64
 * frames long, a 64-column tile of the conv holds whole rows and the normalisation runs INSIDE the conv's epilogue (one launch;
 * avc_tuning.conv_in_fuse); otherwise the conv launch is followed by the row kernel.  *fused (may be NULL) reports which happened. */
int avc_conv1d_in_fwd(const float* x, long sxb, long sxc, int sxt, int B, int Cin, int Tin, const float* wp, const float* bias, int Cout, int KS,
                      int stride, int ops, float* y, const float* cond, long cond_sb, int cond_off, int relu, const float* res, int res_mode,
                      int Tres, float* out, float* mean, float* rstd, int* fused, void* stream);
/* ... and its autograd counterpart one layer up: g = conv1d_input_grad(dy) [+ resT(res): res_mode 1 identity, 3 pool^T, 4 up^T] is the gradient
 * wrt the OUTPUT of an InstanceNorm / AdaIN / activation layer whose saved forward rows are y / mean / rstd ([B][Cin][Tin] contiguous); the call
 * returns the gradient wrt that layer's INPUT rows in dy_out, and dbeta / dgamma in dcond (avc_instnorm_bwd's layout).  One launch where the
 * input-gradient tile holds whole rows (Tin = 16 / 32 / 64: the normalisation's backward runs in the epilogue), two otherwise.  g_out (may be
 * NULL when fused): g itself, for callers that read it again (the skip path of a block). */
int avc_conv1d_dgrad_in_bwd(const float* dy, long syb, long syc, int syt, int yps, int B, int Cout, int Tdy, const float* wpd, int Cin, int KS,
                            int stride, int Tin, float* g_out, const float* res, int res_mode, int Tres, const float* y, const float* mean,
                            const float* rstd, const float* cond, long cond_sb, int cond_off, int relu, float* dy_out, float* dcond,
                            long dcond_sb, int dcond_off, int* fused, void* stream);

/* ---- loss side of a training step over utterances of DIFFERENT lengths (csrc/ragged_loss.hip) ----
 * Shared by the four calls below.  Latent blocks: sample s of muls / d_muls is a [2 c][Tz[s]] block (frames contiguous; the c mu rows, then
 * the c log_sigma rows) at float offset 2 c offz[s]; sample s of z / eps / d_z is a [c][Tz[s]] block at c offz[s] -- the layouts of the ragged
 * plans' ws["muls"] and ws["d_z"] regions.  Tz_dev / offz_dev are DEVICE int32 tables of S entries the caller built (offz = prefix sums of
 * Tz, every Tz[s] >= 1); Tz_max >= every Tz[s] sizes the grid.  fp32 only.  Each call ONLY ENQUEUES on `stream`: no allocation, no copy from
 * the host, no synchronisation -- graph-capture safe.  No atomics, a fixed summation order: two calls give identical bits.  0 on success,
 * -1 for a null argument (eps alone may be NULL) or a bad count (S, N outside 1..65535; a length bound, c, M, n_rec or n_kl below 1). */
/* z = mu + exp(log_sigma / 2) * eps (model.py:383-384; the uniform engine's expression); eps NULL: z = mu.  OVERWRITES the c sum(Tz) floats of
 * z, nothing else. */
int avc_reparam_ragged(const float* muls, const float* eps, int S, const int* Tz_dev, const int* offz_dev, int Tz_max, int c, float* z,
                       void* stream);
/* L1 + KL loss (solver.py:84-86) on packed rows, and d(loss_rec * lambda_rec)/d(dec).  x: utterance j is rows [T[j]][M] (mel bins contiguous)
 * at row xoff[j] (xoff = prefix sums of T); dec / d_dec: block j is [M][out_len[j]] (frames contiguous) at float offset out_off[j] from the
 * pointer passed (avc_plan_ragged_out's offsets minus the first), out_len[j] >= T[j] >= 1: frames t < T[j] count, the crop tail
 * T[j] <= t < out_len[j] is ignored.  T_dev / xoff_dev / out_len_dev (int32) and out_off_dev (int64) are DEVICE tables of N entries;
 * T_max >= every out_len[j].  Latent block j (above; S = N) feeds the KL term.  n_rec = M sum(T), n_kl = c sum(Tz) -- or,
 * on a data-parallel rank, those counts over ALL ranks' utterances: the rank then produces its share of the global means and of their
 * gradient, and the shares add up (likewise lambda_kl_over_n of avc_latent_bwd_ragged).
 * OVERWRITES every element of every d_dec block exactly once: lambda_rec / n_rec (divided in double, rounded once) times sign(dec - x) for
 * t < T[j], 0 in the crop tail; losses[0] = mean |dec - x| over the n_rec kept elements, losses[1] = 0.5 mean(exp(ls) + mu^2 - 1 - ls)
 * over the n_kl latent elements; and the avc_loss_ragged_ws_floats(N, T_max) floats of ws (partial sums; -1 for a bad count). */
long avc_loss_ragged_ws_floats(int N, int T_max);
int avc_loss_ragged(const float* dec, const int* out_len_dev, const long* out_off_dev, const float* x, const int* T_dev, const int* xoff_dev, int N,
                    int M, int T_max, const float* muls, const int* Tz_dev, const int* offz_dev, int c, long n_rec, long n_kl, float lambda_rec,
                    float* d_dec, float* losses, float* ws, void* stream);
/* d(loss)/d(mu | log_sigma) from the KL term and from d_z = d(loss)/d(z): d_mu = lambda_kl_over_n mu + d_z, d_ls = lambda_kl_over_n 0.5
 * (exp(ls) - 1) + d_z eps 0.5 exp(ls / 2) (the uniform engine's expressions; lambda_kl_over_n = lambda_kl / n_kl); eps NULL (z = mu): no
 * second term of d_ls.  Products and sums are rounded one by one (no fused multiply-add).  OVERWRITES the 2 c sum(Tz) floats of d_muls,
 * nothing else. */
int avc_latent_bwd_ragged(const float* muls, const float* eps, const float* d_z, int S, const int* Tz_dev, const int* offz_dev, int Tz_max, int c,
                          float lambda_kl_over_n, float* d_muls, void* stream);

/* ---- device-side feed of the ragged step (csrc/ragged_feed.hip): whole utterances, or crops of them, out of the HBM-resident corpus
 * [n_rows][M] (fp32, mel bins contiguous: the corpus of avc_gather_segments) into the frame-major packed block the ragged grad plans and
 * avc_loss_ragged read as x: out[(xoff[j] + t) M + m] = corpus[(starts[j] + t) M + m] for t < T[j].  T_dev / xoff_dev are the DEVICE int32
 * tables of N entries avc_loss_ragged takes (xoff = prefix sums of T), starts_dev a DEVICE int64 table of N first rows; T_max >= every T[j]
 * sizes the grid.  A segmented copy: 16 bytes per lane for an utterance whose run starts on a 16-byte boundary on both sides (starts[j] M
 * and xoff[j] M multiples of 4, both pointers 16-byte aligned), 4 bytes per lane otherwise; the bits are the corpus's either way.
 * READS rows starts[j] .. starts[j] + T[j] - 1 and nothing else, OVERWRITES the M sum(T) floats of out and nothing else; an utterance whose
 * rows are not all inside [0, n_rows) is skipped as a whole (nothing read, its block left as it was): the caller validates its starts.
 * ONLY ENQUEUES on `stream`: no allocation, no copy from the host, no synchronisation -- graph-capture safe.  0 on success, -1 for a null
 * pointer or a bad count (N outside 1..65535; n_rows, M or T_max below 1). */
int avc_gather_utterances(const float* corpus, long n_rows, int M, const long* starts_dev, const int* T_dev, const int* xoff_dev, int N, int T_max,
                          float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AVC_HIP_H */
