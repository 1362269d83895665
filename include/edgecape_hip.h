/*
 * edgecape_hip.h — C ABI of libedgecape_hip.so: the MI355X (gfx950) implementation of the
 * EdgeCape inference hot path (reference: orhir/EdgeCape `EdgeCape.forward_test`).
 *
 * The reference is pure Python/PyTorch and has NO FFI boundary; this header is the
 * boundary the build introduces.  Each entry point names the reference interface it stands in for:
 *
 *   ec_create / ec_load_tensor / ec_finalize
 *       EdgeCape.__init__ + mmcv load_checkpoint      EdgeCape/models/detectors/EdgeCape.py:28-45, test.py:120-124
 *       tensor names = the reference's state_dict keys (encoder_query.* = upstream dinov2 names,
 *       keypoint_head_module.* = SURVEY Appendix B)
 *   ec_backbone       EdgeCape.extract_features       EdgeCape.py:186-191  (dinov2 get_intermediate_layers(n=1, reshape=True))
 *   ec_head           TwoStageHead.forward            EdgeCape/models/keypoint_heads/head.py:161-222
 *                     (+ SkeletonPredictor.forward    keypoint_heads/skeleton.py:58-161,
 *                        TwoStageSupportRefineTransformer.forward  keypoint_heads/encoder_decoder.py:183-260)
 *   ec_forward        EdgeCape.predict                EdgeCape.py:165-184 (backbone x(1+S) + head), device-side part of forward_test
 *   ec_op_*           single fused ops, exported for the parity tests (each vs a torch fp32 reference)
 *
 * Conventions
 *   - plain C types only; every pointer named *_dev is DEVICE memory owned by the caller
 *     (e.g. torch tensor .data_ptr()); weights/workspace are owned by the library.
 *   - return 0 on success, negative ec_status on failure; ec_last_error() gives the text.
 *     No exceptions cross the ABI.  No hidden synchronisation: work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the legacy default stream).
 *   - a handle is not thread-safe; use one handle per stream.  ec_forward / ec_head fork internal helper streams (support
 *     lane, image lane, decoder helper lane) off `stream` and join them back before returning control of `stream`'s order:
 *     everything the call enqueues is complete when `stream` reaches the end of the call's work (ec_forward_pipelined is the
 *     one exception, see there).
 *   - layouts: images NCHW fp32; heatmaps [bs,K,hm,hm] fp32; features token-major [n,HW,C] fp32
 *     (EC_LAYOUT_TOKENS) or the reference's NCHW (EC_LAYOUT_NCHW).
 */
#ifndef EDGECAPE_HIP_H
#define EDGECAPE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ec_model* ec_handle;

enum ec_status {
  EC_OK = 0,
  EC_ERR_ARG = -1,       /* bad argument / shape */
  EC_ERR_HIP = -2,       /* HIP runtime error */
  EC_ERR_STATE = -3,     /* call order (e.g. forward before finalize), missing tensor */
  EC_ERR_NAME = -4,      /* unknown tensor name */
  EC_ERR_NODEVICE = -5   /* no gfx950 device visible */
};

enum ec_precision {
  EC_F32 = 0,     /* fp32 operands, exact products (v_mfma_f32_32x32x2_f32) */
  EC_BF16 = 1,    /* bf16 operands, fp32 accumulate */
  EC_BF16X3 = 2,  /* fp32 data, each operand split into hi+lo bf16, 3 bf16 MFMAs per product: ~2^-17 relative.  Backbone AND head in this
                     precision were the tolerance-conforming mode of rounds 2-5 (0 / 1 / 1 / 1 argmax flips of 19 288 / 20 293 / 19 699 /
                     9 645 valid keypoints on cfg1 / 2 / 4 / 5, max |d kpt| <= 1.1e-5 otherwise; profiles/r05_conformance_*bf16x3*.json); as a
                     HEAD precision it still is.  As a backbone precision the block GEMMs run K-concatenated on the 16-bit 8-phase
                     kernel: activations as bf16 [hi | lo] planes written by their producers, weights [W_hi | W_lo], one GEMM of depth
                     3 K per Linear.  (fp16 planes instead of bf16 ones were measured at scale in round 6 and not adopted:
                     profiles/r06_conformance_fp16planes_*.json) */
  EC_F16 = 3,     /* IEEE fp16 operands (11 significand bits, same MFMA rate as bf16), fp32 accumulate: the backbone mode that
                     keeps output_kpts inside the 1e-3 tolerance at bf16 speed (backbone only) */
  EC_MIXED = 4,   /* head only: EC_BF16X3 everywhere the proposal generator's argmax depends on (input projections, support pooling,
                     encoder, proposal generator - encoder_decoder.py:91-110 is the path's one discontinuity) and in the small MLPs;
                     single-pass fp16 MFMAs (fp32 data rounded to fp16 operands, fp32 accumulate) in the Linear layers AND the
                     attentions of the skeleton head (skeleton.py:58-161) and of the decoder layers (encoder_decoder.py:584-651),
                     whose image K|V are also stored as fp16 - all of which only move the output continuously.  With the fp16 backbone
                     (bench.py's default): 11 / 12 / 17 / 14 argmax flips of 19 288 / 20 293 / 19 699 / 9 645 valid keypoints on cfg1 / 2 /
                     4 / 5 (512 / 512 / 512 / 256 disjoint pairs), max |d kpt| on flip-free samples 2.4e-4 / 2.0e-4 / 1.6e-4 / 1.6e-4
                     (profiles/r05_conformance_*fp16_mixed.json, re-measured as r06_conformance_*fp16_mixed.json) */
  EC_F16X2 = 5    /* backbone only (round 6): fp32 data, TWO MFMA units per product instead of the three of EC_BF16X3 -
                     a W ~ a_hi W_hi in fp16 MFMAs plus BOTH correction terms a_lo W_hi + a_hi W_lo in ONE block-scaled FP8 pass
                     (v_mfma_scale_f32_16x16x128_f8f6f4: activations e5m2 with fixed power-of-two scales, weights e4m3 with one static
                     scale per tensor and plane), ~2^-14 relative.  Rows of K values travel as [K x fp16 | K x e5m2 | K x e5m2] (4 K
                     bytes), written by their producers (LayerNorm, attention, the fc1 epilogue).  Needs embed_dim % 128 == 0.  Its GEMMs
                     run on ONE kernel whatever the batch, so an image's features do not depend on the batch it rides in.  With the
                     EC_BF16X3 head this is the tolerance-conforming fast mode since round 6: 0 / 2 / 1 / 1 argmax flips of ~20 000 valid
                     keypoints on cfg1 / 2 / 4 / 5 at scale, 1 on planted activation outliers, max |d kpt| <= 2.2e-5 on every flip-free
                     sample (profiles/r06_conformance_*fp16x2_bf16x3.json), at ~1.2 x the pairs/s of EC_BF16X3 / EC_BF16X3 */
};
enum ec_dtype { EC_DT_F32 = 0, EC_DT_F16 = 1, EC_DT_BF16 = 2, EC_DT_F64 = 3 };
enum ec_layout { EC_LAYOUT_TOKENS = 0, EC_LAYOUT_NCHW = 1 };

typedef struct ec_config {
  int32_t embed_dim;          /* backbone width C: 384 / 768 / 1024 */
  int32_t depth;              /* 12 / 24 */
  int32_t num_heads;          /* C / 64 */
  int32_t image_size;         /* input HEIGHT, e.g. 224 / 256 / 384 (the width too unless image_width is set); token grid rows
                                 gh = image_size / patch (floor) */
  int32_t patch;              /* 14 */
  int32_t num_kpts;           /* K keypoint slots, 1..256: 100 in the shipped configs (configs/test/1shot_split1.py:31), the number of clicked
                                 points in the demo (gradio_utils/utils.py:142-148) */
  int32_t d_model;            /* 256 */
  int32_t nhead;              /* 8 */
  int32_t enc_layers;         /* 3 */
  int32_t dec_layers;         /* 3 */
  int32_t skel_layers;        /* 3 */
  int32_t ffn_dim;            /* transformer dim_feedforward F_d = 384 */
  int32_t skel_ffn_dim;       /* SkeletonPredictor dim_feedforward F_s (= embed_dim) */
  int32_t max_hops;           /* 4 */
  int32_t heatmap_size;       /* 64 */
  int32_t max_shots;          /* S_max */
  int32_t max_batch;          /* bs_max (pairs per call) */
  int32_t backbone_precision; /* ec_precision: operand type of the backbone MFMA GEMMs/attention (fp32 accumulate always) */
  int32_t head_precision;     /* EC_F32, EC_BF16X3 or EC_MIXED: GEMM operand handling in the head (LayerNorm / softmax statistics stay fp32) */
  int32_t image_width;        /* input WIDTH; 0 = square (image_size).  The reference takes any img.shape[-2:] (EdgeCape.py:143); token
                                 grid columns gw = image_width / patch.  (ABI version 4) */
  /* (ABI version 5) the model variants of the reference's three training stages (run.py:44-101); 0 / 0 = the shipped test configs */
  int32_t gt_skeleton;        /* 1: SkeletonPredictor(learn_skeleton=False): adj = the normalised ground-truth adjacency of the skeleton
                                 edges, no SkeletonPredictor layers, no Markov stack (skeleton.py:70-74; attn_adj_dev is not written) */
  int32_t no_attn_bias;       /* 1: the decoder layers' self-attention adds no Markov bias (transformer attn_bias=False: nn.MultiheadAttention,
                                 encoder_decoder.py:551-560, 605-612 - its fused in_proj keys are loaded as q / k / v_proj; implied by
                                 gt_skeleton: bias_attn.py:188 skips the bias when there is no stack) */
} ec_config;

typedef struct ec_outputs {
  float* output_kpts_dev;        /* [dec_layers, bs, K, 2]   head.py:222 */
  float* initial_proposals_dev;  /* [bs, K, 2]               encoder_decoder.py:87-89 (proposal_for_loss) */
  float* similarity_map_dev;     /* [bs, K, gh, gw]          encoder_decoder.py:75 */
  float* adj_dev;                /* [bs, 2, K, K]            skeleton.py:142 */
  float* attn_adj_dev;           /* optional (may be NULL): [max_hops+1, bs, K, K]  skeleton.py:152-161 */
  float* out_points_dev;         /* optional (may be NULL): [dec_layers+1, bs, K, 2] encoder_decoder.py:357,403 */
} ec_outputs;

const char* ec_last_error(void);
/* ABI version of the library (EC_ABI_VERSION of the header it was built from): bumped whenever a struct layout, an enum value, the set of entry points
   or a signature changes, so a binding can refuse a stale prebuilt library instead of calling it with mismatched layouts. */
#define EC_ABI_VERSION 7   /* 6 (round 6): ec_precision EC_F16X2, ec_op_linear_x2; 7: ec_op_attention_ex, ec_op_layernorm_ex */
int ec_version(void);
/* sizeof(ec_config) / sizeof(ec_outputs) as the library was compiled: a binding compares them with its own mirrors. */
int ec_abi_sizes(int* config_bytes, int* outputs_bytes);

int ec_create(const ec_config* cfg, ec_handle* out);
int ec_destroy(ec_handle h);

/* Copy one host tensor into the model. `name` is the reference state_dict key. */
int ec_load_tensor(ec_handle h, const char* name, const void* host_ptr, const int64_t* shape, int ndim, int dtype);
/* Positional table for the backbone, ALREADY interpolated to [1+g*g, C] fp32 (host). */
int ec_set_pos_embed(ec_handle h, const float* host_table, int64_t rows, int64_t cols);
/* Check completeness, build derived tables (folded projections, sine tables, bf16 copies). */
int ec_finalize(ec_handle h);

/* n_img images [n_img,3,H,W] fp32 -> features [n_img,HW,C] (tokens) or [n_img,C,g,g] (NCHW). */
int ec_backbone(ec_handle h, const float* img_dev, int n_img, float* feat_dev, int layout, void* stream);

/* Head on given features. feature_s_dev/target_s_dev: arrays (host) of S device pointers.
 * mask_s_dev [bs,K] fp32 (product of target weights, EdgeCape.py:175-177).
 * edges: host int32 pairs (0-based, < K), edge_offsets: host int32 [bs+1] offsets in PAIRS. */
int ec_head(ec_handle h, const float* feature_q_dev, const float* const* feature_s_dev, int layout,
            const float* const* target_s_dev, const float* mask_s_dev, const int32_t* edges,
            const int32_t* edge_offsets, int bs, int S, void* stream, const ec_outputs* out);

/* Whole device-side forward_test: backbone on query + S supports, then the head. */
int ec_forward(ec_handle h, const float* img_q_dev, const float* const* img_s_dev,
               const float* const* target_s_dev, const float* mask_s_dev, const int32_t* edges,
               const int32_t* edge_offsets, int bs, int S, void* stream, const ec_outputs* out);

/* Pipelined forward for back-to-back batches (the reference's evaluation loop, EdgeCape/apis/test.py:31-33, only needs the results
 * in order).  Same arguments and results (bit for bit) as ec_forward, different completion rule: only the backbone runs on `stream`;
 * the WHOLE head of call i - ~1.7 ms of dependent small kernels that cannot fill the chip - is enqueued on streams owned by the
 * library and is NOT joined: it runs beside the backbone of call i+1 (a head waits for the previous call's head, which owns the head
 * workspace, on those streams - never on `stream`).  What reads the caller's heatmaps / masks (adjacency build, pooling tap lists)
 * needs no backbone output and runs beside the call's OWN backbone.
 *   - ALL outputs of call i are complete once a stream has passed an ec_pipeline_flush(h, that_stream) issued after call i and before
 *     the next pipelined call, or once `stream` has passed the first kernel of any other entry point of this handle that touches the
 *     head (ec_forward, ec_head, ec_support_encode, ec_forward_cached wait for a pending head on `stream`);
 *   - the output buffers of call i must stay valid until then, and consecutive calls must not share output buffers if the caller
 *     reads call i's results after enqueuing call i+1; inputs may be released as for ec_forward (when `stream` has passed the call:
 *     the library's last read of the images, heatmaps and masks lies before that point).
 * ec_pipeline_flush enqueues, on ANY stream, a wait for the head of the most recent pipelined call (no host synchronisation):
 * a copy stream can so fetch call i's results without waiting for call i+1's backbone.
 * EC_PIPE_FULL=0 keeps the first form of round 3 (only the decoder phase is deferred; the other outputs are then complete when
 * `stream` has passed the call).  Measured on cfg2: 4770 pairs/s through ec_forward, 5135 with the decoder phase
 * deferred, 5235 with the whole head deferred (one box, interleaved). */
int ec_forward_pipelined(ec_handle h, const float* img_q_dev, const float* const* img_s_dev,
                         const float* const* target_s_dev, const float* mask_s_dev, const int32_t* edges,
                         const int32_t* edge_offsets, int bs, int S, void* stream, const ec_outputs* out);
int ec_pipeline_flush(ec_handle h, void* stream);

/* ---- support-side episode cache --------------------------------------------------------
 * The reference pairs ONE support set with 15 queries (EdgeCape/datasets/datasets/mp100/test_dataset.py:93-97) and
 * recomputes the support backbone features, the pooled support tokens (head.py:175-188) and the whole SkeletonPredictor
 * (skeleton.py:58-161; it has no query input, head.py:196-200) for every pair.  ec_support_encode does that work once
 * per episode; ec_forward_cached then runs the query side only (query backbone, input_proj, encoder, proposal generator,
 * decoder, kpt branches) for a batch of queries, query b using episode episode_of_query[b].  Results are identical to
 * ec_forward on the expanded (support, query) pairs. */
typedef struct ec_support* ec_support_t;
/* A cache of max_episodes SLOTS, one episode each (state per slot: support tokens [K,d], masks, adj [2,K,K], Markov stack
 * [max_hops+1,K,K]: ~0.4 MB at K = 100). */
int ec_support_create(ec_handle h, int max_episodes, ec_support_t* out);
int ec_support_destroy(ec_support_t s);
/* Encode n_episodes (<= max_batch) episodes into slots 0 .. n_episodes-1; the other slots become empty. */
int ec_support_encode(ec_handle h, ec_support_t s, const float* const* img_s_dev, const float* const* target_s_dev,
                      const float* mask_s_dev, const int32_t* edges, const int32_t* edge_offsets, int n_episodes, int S,
                      void* stream);
/* Query side for bs queries, query b against the episode in slot episode_of_query[b] (host array). */
int ec_forward_cached(ec_handle h, ec_support_t s, const float* img_q_dev, const int32_t* episode_of_query, int bs,
                      void* stream, const ec_outputs* out);
/* Streaming form (ABI 5): the reference's evaluation order - every episode followed by its 15 queries, test_dataset.py:86-99 -
 * cut into calls of bs queries.  A call ENCODES the n_new episodes that start in it (arguments as ec_support_encode, plus
 * new_slots: host [n_new], the cache slot each one is written to - distinct, < max_episodes; a slot is free again once the last
 * query of its old episode has been passed to a call) AND runs the query side for bs queries, query b against slot
 * slot_of_query[b] (host [bs]; a slot filled by an earlier call or by this one).  The support images of the new episodes ride in
 * the SAME backbone pass as the queries (one pass over bs + n_new * S images: no small, latency-bound support pass), with
 * bs + n_new * S <= (1 + max_shots) * max_batch, bs <= max_batch, n_new <= max_batch.  n_new = 0 (queries only) and bs = 0
 * (encode only; out may be NULL) are allowed.  Results are identical to ec_support_encode + ec_forward_cached, i.e. to ec_forward
 * on the expanded pairs.
 * pipelined = 0: complete when `stream` has passed the call (ec_forward's rule).  pipelined != 0: ec_forward_pipelined's rule -
 * only the backbone runs on `stream`; the whole head (support lane of the new episodes, query lane of the queries) runs on the
 * library's streams beside the NEXT call's backbone; outputs are complete after ec_pipeline_flush, and consecutive calls must not
 * share output buffers. */
int ec_forward_episodes(ec_handle h, ec_support_t s, const float* const* img_s_dev, const float* const* target_s_dev,
                        const float* mask_s_dev, const int32_t* edges, const int32_t* edge_offsets, const int32_t* new_slots,
                        int n_new, int S, const float* img_q_dev, const int32_t* slot_of_query, int bs, void* stream,
                        const ec_outputs* out, int pipelined);

/* ---- on-device input pipeline (no model handle needed) -----------------------------------
 * ec_preprocess_images = TopDownAffineFewShot (cv2.warpAffine INTER_LINEAR, constant-0 border;
 *   EdgeCape/datasets/pipelines/top_down_transform.py:35-58) + ToTensor + NormalizeTensor (configs/test/1shot_split1.py:
 *   119-125) for n RGB uint8 HWC images already on the device: src_dev = host array of n device pointers, src_hw = host
 *   [n,2] (rows, cols), src_pitch = host [n] row pitches in bytes or NULL (= cols*3), inv_affine = host [n,6] dst->src 2x3
 *   matrices (get_affine_transform(center, scale, rot, size, inv=True)), out_dev [n,3,out_size,out_size] fp32.
 *   Interpolation is exact float bilinear on un-rounded pixel values (NOT what cv2 computes: see ec_preprocess_images_cv2,
 *   the default of edgecape_amd.preprocess).
 * ec_msra_targets = TopDownGenerateTargetFewShot._msra_generate_target, biased branch (top_down_transform.py:165-194):
 *   joints_dev [n,K,2] model-input pixels, visible_dev [n,K] -> target_dev [n,K,hm,hm], weight_dev [n,K]; gauss_host = the
 *   7x7 float32 gaussian computed on the host as the reference does (np.exp on float32), so the result is bit-exact. */
int ec_preprocess_images(const uint8_t* const* src_dev, const int32_t* src_hw, const int64_t* src_pitch,
                         const float* inv_affine, int n, int out_size, const float* mean, const float* stdv,
                         float* out_dev, void* stream);
/* The same stage with cv2.warpAffine's own arithmetic on the uint8 pixels (the reference's call, top_down_transform.py:55-58):
 *   fwd_affine = host [n,6] FLOAT64 src->dst matrices exactly as the reference hands them to cv2.warpAffine
 *   (get_affine_transform(center, scale, rot, size)); the library inverts them as cv::warpAffine does, quantises the source
 *   coordinate to 1/32 px through OpenCV's 1/1024-px fixed point, weights the four taps with the int16 bilinear table
 *   (sum 32768), rounds (acc + 2^14) >> 15 to uint8, then ToTensor / NormalizeTensor in float32: out = (u8 / 255 - mean) / std.
 *   cv2 itself is absent from the build image: pinned to OpenCV's published algorithm (imgwarp.cpp, classic fixed-point path)
 *   through the numpy restatement oracle/pipeline_oracle.py::cv2_warp_affine_linear_u8, bit for bit. */
int ec_preprocess_images_cv2(const uint8_t* const* src_dev, const int32_t* src_hw, const int64_t* src_pitch,
                             const double* fwd_affine, int n, int out_size, const float* mean, const float* stdv,
                             float* out_dev, void* stream);
int ec_msra_targets(const float* joints_dev, const float* visible_dev, int n, int K, int image_size, int heatmap_size,
                    int sigma, const float* gauss_host, float* target_dev, float* weight_dev, void* stream);

/* Copy a named intermediate of the LAST forward/head call to a host fp32 buffer (tests only; synchronises). */
int ec_debug_read(ec_handle h, const char* name, float* host_out, int64_t max_elems, int64_t* n_elems);

/* Measurement hook for bench.py (§ roofline): when enabled, a HIP event pair brackets every launch of the
 * backbone QKV GEMM (the north-star kernel) on the caller's stream; ec_profile_read synchronises on them and
 * returns the summed kernel time and the number of launches since the last ec_profile(h, 1, n).
 * enable = 2 (round 3): SAMPLED - one launch per backbone pass is bracketed, the block index rotating with the pass
 * (pass p times block p % depth), so that every block is covered over `depth` passes.  An event pair costs the stream
 * two ~6 us barrier packets around the launch (profiles/r03_step_trace.txt: 12 x 12 us = 2 % of a cfg2 step when every
 * launch is bracketed); the sampled form keeps the timed region honest to what an unprofiled run does. */
int ec_profile(ec_handle h, int enable, int max_launches);
int ec_profile_read(ec_handle h, float* total_ms, int* launches);

/* ---- single ops (parity tests / microbenchmarks) -------------------------------------------- */
/* C[M,N] = epilogue(A[M,K] @ W[N,K]^T): precision EC_F32 -> fp32 operands, EC_BF16 -> operands are
 * rounded to bf16 on device first (EC_MIXED: the single-pass fp16 form of the mixed head precision).  act: 0 none, 1 relu, 2 gelu(erf).  bias/gamma/resid may be NULL.
 * EC_F16X2 (ec_op_linear_x2) or an unknown precision is EC_ERR_ARG. */
int ec_op_linear(const float* A_dev, const float* W_dev, const float* bias_dev, const float* gamma_dev,
                 const float* resid_dev, float* C_dev, int M, int N, int K, int act, int precision, void* stream);
/* The block GEMMs of the backbone as the model runs them: operands rounded to the 16-bit format of `precision` (EC_BF16 / EC_F16) on
 * device, 16-BIT OUTPUT (bit patterns) with the fused epilogue act(A @ W^T + bias) * gamma - the output kinds of the 8-phase kernel
 * (ec_gemm8.hip: qkv / proj: bias; fc2: bias, LayerScale; fc1: bias, GELU; dinov2 Attention / Mlp / LayerScale).  gamma may be NULL,
 * act 0 or 2 (not both gamma and act).  The launch is repeated `repeats` times back to back (race screens). */
int ec_op_linear_h16(const float* A_dev, const float* W_dev, const float* bias_dev, const float* gamma_dev, uint16_t* C_dev, int M, int N,
                     int K, int act, int precision, int repeats, void* stream);
/* The block GEMMs of the EC_F16X2 backbone as the model runs them (ec_gemm8.hip, X2 instantiations): A [M,K] and W [N,K] fp32 on device
 * are packed into fp16x2 rows ([K x fp16 | K x FP8 | K x FP8]: activations e5m2 with fixed scales, weights e4m3 with one static
 * power-of-two scale per plane) and multiplied as a_hi W_hi (fp16 MFMAs) + a_lo8 W_hi8 + a_hi8 W_lo8 (block-scaled FP8 MFMAs).
 *   act = 0, gamma NULL: C_dev [M,N] fp32 = A W^T + bias                                   (QKV)
 *   act = 0, gamma:      C_dev = (A W^T + bias) * gamma + C_dev, in place                  (proj / fc2: LayerScale + residual)
 *   act = 2:             planes_dev [M, 4 N] bytes = fp16x2 rows of gelu(A W^T + bias)     (fc1); C_dev unused
 * K % 128 == 0, N % 16 == 0, N >= 256, any M.  Repeated `repeats` times back to back; *ms (may be NULL) = mean launch time. */
int ec_op_linear_x2(const float* A_dev, const float* W_dev, const float* bias_dev, const float* gamma_dev, float* C_dev, void* planes_dev,
                    int M, int N, int K, int act, int repeats, void* stream, float* ms);
/* Same GEMM on operands already in the precision's storage type (bf16 as uint16_t bit patterns), repeated
 * `iters` times; returns mean kernel time in ms via *ms (HIP events on `stream`).  Used by bench.py roofline. */
int ec_op_gemm_bench(const void* A_dev, const void* W_dev, const float* bias_dev, void* C_dev, int M, int N, int K,
                     int precision, int iters, void* stream, float* ms);
/* C[b] = A[b] @ op(B[b]) for b < batch; A [M,K], B [K,N] (transB = 0) or [N,K] (transB = 1), C [M,N], fp32, exact-fp32 MFMA:
 * the per-sample contractions of the head (support pooling head.py:181-184, cosine adjacency skeleton.py:136-137, Markov powers
 * :159, GCN aggregation encoder_decoder.py:517, similarity map :75). */
int ec_op_bgemm(const float* A_dev, const float* B_dev, float* C_dev, int batch, int M, int N, int K, int transB, void* stream);
int ec_op_layernorm(const float* x_dev, const float* w_dev, const float* b_dev, float* y_dev, int rows, int cols,
                    float eps, void* stream);
/* LayerNorm with every form the model launches (the fields of ec_ops.h LnP as plain arguments), straight to the kernel dispatch:
 *   y = LayerNorm(x') * w + b over `cols`, x' = x, or (x + add) + add2 in fp32 when add is set (16-bit branch rows of stride ldadd in
 *   add_fmt's format: 1 bf16, 2 fp16, 0 = the output's); x' is written to xsum when xsum is not NULL (xsum may be x, same stride ldx).
 *   out_fmt: 0 fp32, 1 bf16, 2 fp16 (saturated at +-65504), 3 bf16 split [hi | lo] (planes cols apart, ldy >= 2 cols, no add),
 *   6 fp16x2 row [fp16 | e5m2 lo8 | e5m2 hi8] (ldy >= 2 cols 16-bit units, no add).  drop_period > 0: input row n * P + t goes to output
 *   row n * (P - 1) + t - 1, rows t = 0 are dropped.  y2 (fp32 output only, may be NULL): an fp16 copy of y, row stride ldy2.
 *   Strides in elements of the buffer's type; cols % 4 == 0, cols <= 1024. */
int ec_op_layernorm_ex(const float* x_dev, int64_t ldx, void* y_dev, int64_t ldy, int out_fmt, const float* w_dev, const float* b_dev,
                       int rows, int cols, float eps, int drop_period, const void* add_dev, const void* add2_dev, int64_t ldadd,
                       int add_fmt, float* xsum_dev, void* y2_dev, int64_t ldy2, void* stream);
/* Row-chain kernel of the head (ec_chain.hip; bf16x3 arithmetic), up to three stages over `rows` token rows in ONE launch:
 *     x1   = LayerNorm_1(resid + X @ W1^T + b1)                              X [rows,K1], W1 [256,K1]  -> x1_out [rows,256]
 *     out2 = act2([x1 | cat] @ W2^T + b2 + table[row % period])              W2 [N2, 256 + Kcat]       -> out2 [rows,N2]
 *     x3   = LayerNorm_3(x1 + out2 @ W3^T + b3)                              W3 [256, N2]              -> x3_out [rows,256]
 * (transformer.py-style residual blocks: EdgeCape/models/keypoint_heads/encoder_decoder.py:461-483, 596-649).  Weights are plain
 * fp32 [N,K] device arrays (packed inside).  cat / table / the whole third stage (W3 = NULL) are optional; resid may alias x1_out (one workgroup per 32-row slab; a separate resid buffer
 * selects two workgroups per slab that deal the column passes of stage 2 out between them);
 * LayerNorm eps = 1e-5; act2: 0 none, 1 relu, 2 gelu(erf).  K1, Kcat, N2 multiples of 128.  precision: EC_BF16X3, or EC_MIXED for the
 * single-pass fp16 form the skeleton head / decoder layers use under head_precision = EC_MIXED. */
int ec_op_chain(const float* X_dev, int K1, const float* W1_dev, const float* b1_dev, const float* resid_dev, const float* ln1_w_dev,
                const float* ln1_b_dev, float* x1_out_dev, const float* cat_dev, int Kcat, const float* W2_dev, const float* b2_dev,
                int N2, int act2, const float* table_dev, int period, float* out2_dev, const float* W3_dev, const float* b3_dev,
                const float* ln3_w_dev, const float* ln3_b_dev, float* x3_out_dev, int rows, int precision, void* stream);
/* softmax(q k^T * hd^-0.5 + bias, key mask) v ; q [B,Lq,H*hd], k,v [B,Lk,H*hd]; kmask [B,Lk] uint8 (1 = masked) or NULL;
 * bias [B,H,Lq,Lk] or NULL.  precision EC_F32, EC_BF16X3, or EC_BF16 / EC_F16 (fp32 data rounded on device, hd = 64, no mask / bias);
 * any other value is EC_ERR_ARG. */
int ec_op_attention(const float* q_dev, const float* k_dev, const float* v_dev, const uint8_t* kmask_dev,
                    const float* bias_dev, float* o_dev, int B, int H, int Lq, int Lk, int hd, int precision,
                    void* stream);
/* The same attention with every field of the kernel's problem (ec_common.h AttnP) as the model passes it: operands as the caller's bytes
 * (no conversion pass), row strides ld* and batch strides s* in elements of each operand's own type; head h of a row is the hd
 * elements from h * hd.  Key k of batch b is masked when k >= mask_start and kmask[(mask_mod > 0 ? b % mask_mod : b) * mask_len +
 * k - mask_start] != 0 (kmask may be NULL); bias [B,H,Lq,Lk] fp32 or NULL.
 *   mode EC_F32:    fp32 Q/K/V/O, exact fp32 products
 *   mode EC_BF16X3: fp32 Q/K/V/O, each product as three bf16 MFMAs (split)
 *   mode EC_MIXED:  the split kernel's single-pass fp16 form (Q * hd^-0.5, K, V and P rounded to fp16, one fp16 MFMA per product)
 *   mode EC_BF16 / EC_F16: Q/K/V/O all 16-bit (backbone kernel: hd = 64, no mask / bias)
 *   kv16 (split modes, hd = 64): K and V are IEEE fp16.
 *   o_x3 (split modes): 0 fp32 O; 1 bf16 split rows [hi | lo] (planes H * hd apart, ldo / sO in 16-bit units);
 *        3 fp16x2 rows [fp16 | e5m2 lo8 | e5m2 hi8] (ldo / sO in 16-bit units, ldo >= 2 H hd).
 * Apart from the mode and flag values, validates nothing beyond what the kernel dispatch itself enforces. */
int ec_op_attention_ex(const void* q_dev, const void* k_dev, const void* v_dev, void* o_dev, int64_t ldq, int64_t ldk, int64_t ldv,
                       int64_t ldo, int64_t sQ, int64_t sK, int64_t sV, int64_t sO, const uint8_t* kmask_dev, int mask_start,
                       int mask_len, int mask_mod, const float* bias_dev, int B, int H, int Lq, int Lk, int hd, int mode, int kv16,
                       int o_x3, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EDGECAPE_HIP_H */
