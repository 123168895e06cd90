/*
 * vc_engine.h — C ABI of libvcengine.so, the MI355X (gfx950) engine for the
 * VoiceCraft token-infilling decode path.
 *
 * The reference (jasonppy/VoiceCraft) has no FFI: its boundary for this path is
 * three Python methods on an nn.Module plus two tokenizer methods.
 * Each entry point below names the reference interface it replaces; the Python
 * mirror of that interface lives in voicecraft_amd/engine.py and is the only
 * in-tree caller (ctypes).  INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success or a negative
 *     VC_E* code, with a human-readable message available from vc_last_error().
 *   - `*_dev` pointers are device (HBM) pointers owned by the caller; the engine
 *     owns everything it allocates itself and frees it in vc_destroy().
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *   - token tensors are int64, matching the reference's LongTensors.
 *   - one engine per (process, GPU); not thread-safe (the reference is neither:
 *     inference_tts_scale.py:42 runs single-threaded under torch.no_grad()).
 */
#ifndef VC_ENGINE_H
#define VC_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VC_OK 0
#define VC_EINVAL (-1)   /* bad argument / shape (the reference would AssertionError) */
#define VC_ESTATE (-2)   /* call order (e.g. decode before vc_finalize_weights)       */
#define VC_EHIP (-3)     /* a HIP runtime call failed                                 */
#define VC_ECAP (-4)     /* a capacity given at vc_create / by the caller is too small */
#define VC_EMISSING (-5) /* a required weight tensor was never loaded                 */

#define VC_DTYPE_F32 0
#define VC_DTYPE_BF16 1
#define VC_DTYPE_I64 2

#define VC_MAX_CODEBOOKS 8
#define VC_MAX_SPANS 8
#define VC_MAX_SILENCE 8

typedef struct vc_engine vc_engine;

/* Model hyper-parameters = the fields of the reference's pickled `args` Namespace that
 * the inference path reads (models/voicecraft.py:105-185, config.py:55-84), plus the
 * capacities the engine sizes its HBM arenas with. */
/* The token side of the model, accepted and tested ranges (tests/test_gpu_codebooks.py, tests/golden/model_*k*.npz):
 *   n_codebooks K   2..VC_MAX_CODEBOOKS.  K = 1 is refused (VC_EINVAL): the reference's own TTS cuts the shifted prompt with
 *                   [:, :-(n_codebooks-1)] (voicecraft.py:967, :1217), which drops the WHOLE audio prompt at one codebook, so there is
 *                   nothing to be equal to.  (The engine-less pattern entry points below keep K = 1.)  Run against the reference
 *                   at K = 2, 3, 4, 5, 6 and 8.
 *   V               audio_vocab_size + n_special <= 2176 (64 lanes x 34 logits in the sampler).  Run at V = 515, 1028, 1540, 2051,
 *                   2052 and 2176; the sampler alone at every V in {1, 2, 63, 64, 65, 2175, 2176} as well.
 *   head_hidden P   a multiple of 256.  Run at 256, 512, 768 and 1024; 768 has no wide-decode form (steps of 17..64 rows run its
 *                   heads on the weight-stationary kernel). */
typedef struct vc_model_cfg {
  int32_t d_model;          /* args.d_model                                   */
  int32_t nhead;            /* args.nhead                                     */
  int32_t num_layers;       /* args.num_decoder_layers                        */
  int32_t n_codebooks;      /* args.n_codebooks (K), 2..VC_MAX_CODEBOOKS      */
  int32_t audio_vocab_size; /* args.audio_vocab_size (2048)                   */
  int32_t n_special;        /* args.n_special; V = audio_vocab_size+n_special <= 2176 */
  int32_t text_rows;        /* args.text_vocab_size + 1 (voicecraft.py:129)   */
  int32_t head_hidden;      /* audio_vocab_size // 2   (voicecraft.py:183); a multiple of 256 */
  int32_t empty_token;      /* args.empty_token                               */
  int32_t eog;              /* args.eog                                       */
  int32_t audio_pad_token;  /* args.audio_pad_token                           */
  int32_t eos;              /* args.eos, or -1 when the checkpoint has none   */
  int32_t reduced_eog;      /* args.reduced_eog (voicecraft.py:240)           */
  int32_t encodec_sr;       /* args.encodec_sr (50)                           */
  int32_t max_n_spans;      /* args.max_n_spans: rows of mask_embedding       */
  int32_t max_seqs;         /* capacity: concurrent sequences (KV slots)      */
  int32_t max_positions;    /* capacity: cached positions per sequence        */
} vc_model_cfg;

/* Decode controls = the keyword arguments of inference_tts / inference
 * (models/voicecraft.py:908-920, :561-573). */
typedef struct vc_sample_cfg {
  int32_t top_k;            /* <=0: no top-k filter (reference default -100)  */
  float top_p;              /* >=1: no nucleus filter                         */
  float temperature;        /* 1.0: untouched                                 */
  int32_t stop_repetition;  /* <=0: silence-run penalty off                   */
  int32_t n_silence;        /* number of entries used in silence_tokens       */
  int32_t silence_tokens[VC_MAX_SILENCE];
  uint64_t seed;            /* Philox key; stream = (seed, sequence, step, codebook).  The draws follow the
                             * DISTRIBUTION of topk_sampling (voicecraft.py:71-86), not torch's generator stream; ties at
                             * the k-th value survive as in the reference; exact ties at the nucleus boundary are kept or
                             * dropped together (the reference's sort splits them arbitrarily) */
  int32_t use_graph;        /* 1: replay the decode step as a captured hipGraph */
  int32_t poll_every;       /* host polls the done flag every N steps (0 = default 16) */
  int32_t forced_mode;      /* parity hook, meaning of forced_dev: 0 = the step's FINAL tokens (teacher forcing
                             * for logits parity); 1 = the raw draws of topk_sampling (models/voicecraft.py:1033):
                             * the state machine - overrides, termination, best-of-N keep - runs on them */
} vc_sample_cfg;

/* ---- lifecycle ---------------------------------------------------------- */
int vc_create(const vc_model_cfg* cfg, int hip_device, vc_engine** out);
void vc_destroy(vc_engine* e);
const char* vc_last_error(const vc_engine* e); /* e may be NULL: last vc_create error */
const char* vc_version(void);

/* Run-time options of a finalized engine: launch-shape knobs of the decode step, the same ones the VC_* environment
 * variables preset when the engine is created (no reference counterpart: the reference has no such knobs).  Sixteen of them (round 6
 * pruned round 5's 22 to 14 - the prefetch roles and the knobs whose value every measurement had fixed are constants now, the K/V hint is a
 * second value of "nt" - and added two measurement arms, "att_p16" and "hq").  name / value:
 *   "nt"           "mask[,kv]"  mask: the weight matrices streamed with the non-temporal hint (1 QKV, 2 out-proj, 4 FFN-up, 8 FFN-down, 16 / 32
 *                  heads); kv 0 / 1 / 2 = the decode attention's K/V loads carry it never / always / from two rows per step (the separate
 *                  name "attn_nt" of rounds 4-5 is gone)
 *   "finished_rows" rows up to which a several-row decode step keeps whole residual rows instead of split-K slabs (0 = off, max 16);
 *                  "fr_pair" 1 = its FFN down-projection with two k-tiles per MFMA fragment at 2..8 rows;  "att_p16" 1 (default) = bf16 mode: the
 *                  split attention of 2..8-row steps leaves its partial outputs in bf16 for the out-projection's merge;  "hq" 1 (default) = the
 *                  producers of finished rows also store a copy of each row in the compute dtype, centred on the mean its previous LayerNorm
 *                  found, and the LayerNorm-folding consumers read that copy instead of the fp32 rows (widths whose row of the copy is whole
 *                  1 KB requests: d a multiple of 512 in bf16, of 256 in fp32; others keep the fp32 rows)
 *   "fr_one"       ONE-row steps: 1 (default) = the FFN down-projection finishes its row (no split-K slabs), 0 = off;  "qkv_p8" 1 = the
 *                  one-row QKV projection in the same paired form, 2 (default) = also the QKV projection of 2..8 finished rows behind the
 *                  centred copy ("hq"; rows_gemm_qp_k: up to 6 rows at d >= 2048, where 8 rows measured slower);  "attn_fast" 1 = decode attention without per-visit rescaling (bf16: hardware exp2)
 *   "tile_attn"    "k[,min_rows]"  prefill attention kernel (1: 16 query rows per wave; 2: 64 per workgroup, P in registers - bf16,
 *                  head_dim 128, calls whose longest prompt has at least min_rows rows)
 *   "qkv16"        1 = prefill passes and wide decode passes (17..64 rows) run the QKV projection on a 16-channel image of the folded matrix
 *                  instead of the one-row kernels' 12-channel tiles.  The image is packed for engines with max_seqs > 16 (or VC_QKV16=1 at
 *                  creation); without it the option stays 0 and wide steps fall back to the weight-stationary kernel
 *   "wide_heads"   1 (default) = decode steps of 17..64 rows run the prediction heads once on the wide-decode kernel instead of once per 16 rows
 *   "wide_gemm"    1 (default) = the linear layers of 17..64-row steps run on rows_gemm_wd_k / rows_gemm_wds_k (every row tile of the step in flight;
 *                  widths whose K does not split into 8 x {1, 2, 4, 8, 16} k-tiles, and 0, take the weight-stationary rows_gemm_mt_k of rounds 2-5);
 *                  "wd_stage" 1 (default) = that kernel takes X as whole cache lines through a wave-private LDS stage, 0 = MFMA fragments straight from L2
 *   "shrink"       1 (default) = a multi-utterance call re-packs its live sequences onto the rows of a narrower step (next power of two) as the
 *                  others retire; 0 = the step keeps its starting width until the longest sequence ends (rounds 1-5)
 *   "graph_steps"  decode steps captured per hipGraph;  "prefill_rows"  rows per prefill pass (16: decode kernels only)
 *   "w13"          mask (default 5): ONE-row steps of a bf16 engine stream the FFN down-projection (1) and the QKV projection (4) as exact
 *                  13-bit planes of the same bf16 values (low byte, 4-bit exponent code, sign; one base byte per 512-value MFMA fragment:
 *                  13/16 of the bytes, every result bit-identical); any other bit: VC_EINVAL.  Planes are packed at creation unless
 *                  VC_W13=0 (+ 0.81 x the two images); a width whose wave shares are not whole groups of four fragments (FFN-down below
 *                  d = 512, QKV below d = 1024), an fp32 engine, and a matrix of a layer with a fragment whose non-zero exponents span more
 *                  than 30 binades keep the bf16 launch (vc_debug_read "w13_stats": int32 [layer][FFN-down, QKV][state 0 n/a / 1 packed /
 *                  2 refused, fragments refused])
 *   "w8"           mask of the same bits, ONLY on an engine that called vc_request_w8 (default: the requested mask; VC_EINVAL on any other
 *                  engine): those launches stream one OCP E4M3 byte per value + one shift byte per 512-value fragment, half the bytes of the
 *                  image, decoded to the bit-identical bf16 operands (v_cvt_scalef32_pk_bf16_fp8), for matrices whose every fragment lies on
 *                  that grid (value = q . 2^s, q E4M3 and not its NaN code, the value a normal bf16 number or +-0; voicecraft_amd/quant.py
 *                  puts a checkpoint there).  A matrix off the grid is refused and keeps its current launch (vc_debug_read "w8_stats",
 *                  layout of "w13_stats").  Where a matrix has both kinds of planes the w8 bit wins.  The option text ends in |w8=<mask>
 *                  on such an engine only.  Resident memory: + 0.5 x the requested images
 *   "w8r"          mask of the same bits, ONLY on an engine that called vc_request_w8_rows (default: the requested mask; VC_EINVAL on any
 *                  other engine): steps of 2..8 finished rows stream the same planes - the FFN down-projection (1: rows_gemm_frp_w8_k, at
 *                  d = 512, 1024, 2048) and the QKV projection of layers 1.. (4: rows_gemm_qp_w8_k, at d = 2048, up to 6 rows) -, every
 *                  result bit-identical to the image launch; a refused matrix keeps its image launch for that layer.  "w8" stays the
 *                  one-row launches.  The option text ends in |w8=<mask>|w8r=<mask> on such an engine only (vc_debug_w8r_plan says which
 *                  row counts take the form)
 *   "w8m"          1 (FFN-down) plus 8, ONLY on an engine that called vc_request_w8_mid (default: the requested mask; VC_EINVAL on any
 *                  other engine): passes of 9..16 finished rows stream the FFN down-projection from the same planes (rows_gemm_fr_w8_k
 *                  at d = 512, 1024: X in LDS in one piece; rows_gemm_fr2_w8_k at d = 2048: K in two halves - the image kernels' text,
 *                  one decoded fragment feeding two consecutive k-tiles), every result bit-identical to the image launch; a refused
 *                  matrix keeps its image launch for that layer.  Bit 8: also at the row counts the measured win table leaves out (for
 *                  the A/B tool and the tests; vc_debug_w8m_plan says which row counts take the form).  The option text gains
 *                  |w8m=<v> behind |w8=<mask> and, if present, |w8r=<mask>, in front of |w8w=<v>, on such an engine only.  Resident
 *                  memory does not change: nothing more is packed
 *   "w8w"          mask of the same bits plus 8, ONLY on an engine that called vc_request_w8_wide (default: the requested mask; VC_EINVAL
 *                  on any other engine): steps of 17..64 rows stream the FFN down-projection (1) and the QKV projection of every layer
 *                  (4) as E4M3 PAIR planes of their 16-channel images (rows_gemm_wds_w8_k: the staged wide kernel, option "wd_stage" = 1,
 *                  where the K slice a wave owns is 2, 4 or 8 k-tiles) - a pair = two k-tiles of a 16-channel tile = 1 KB of codes +
 *                  two shift bytes (channels 0..7, channels 8..15: two blocks of the same grid) -, every result bit-identical to the
 *                  image launch; a refused matrix keeps its image launch for that layer (vc_debug_read "w8w_stats", layout of
 *                  "w13_stats", pairs refused).  Bit 8: also at the row counts the measured win table leaves out (for the A/B tool and
 *                  the tests; vc_debug_w8w_plan says which row counts take the form).  The option text gains |w8w=<v> behind |w8=<mask>
 *                  and, if present, |w8r=<mask> on such an engine only.  Resident memory: + 0.5 x the two images (7 d^2 bytes per
 *                  layer: + 0.47 GB at giga830M), on engines that can run wide steps (max_seqs > 16)
 *   "w8u"          0 / 2 / 10, ONLY on an engine that called vc_request_w8_up (default 2; VC_EINVAL on any other engine and for any
 *                  other value): steps of 17..64 rows stream the FFN up-projection of every layer (2) as E4M3 pair planes of its
 *                  16-channel image (rows_gemm_wds_w8u_k: the text of rows_gemm_wds_w8_k with the bias + ReLU epilogue; K = d in one
 *                  slice of 2, 4 or 8 k-tiles per wave: d = 512 / 1024 / 2048), every result bit-identical to the image launch; a
 *                  refused layer keeps its image launch (vc_debug_read "w8u_stats": int32 [layer][state, pairs refused]).  10 = 2 + bit
 *                  8: also at the row counts the measured win table leaves out (for the A/B tool and the tests; vc_debug_w8u_plan
 *                  says which row counts take the form).  Independent of "w8w".  Steps of up to 16 rows keep reading the bf16 image
 *                  of the same values.  The option text gains |w8u=<v> right behind |w8w=<v> (or where that would stand) on such an
 *                  engine only.  Resident memory: + 0.5 x the W1 image (4 d^2 + d^2 / 128 bytes per layer: + 0.27 GB at giga830M),
 *                  on engines that can run wide steps (max_seqs > 16)
 *   "w8ur"         0 / 2 / 10, ONLY on an engine that called vc_request_w8_up_rows (default 2; VC_EINVAL on any other engine and for any
 *                  other value): passes of 2..16 finished rows behind a centred copy (option "hq") stream the FFN up-projection of every
 *                  layer (2) from the E4M3 pair planes of its 16-channel image - the planes of "w8u" - (rows_gemm_lnq_w8_k: the text of
 *                  rows_gemm_k<bf16, KTW, PRO_LNQ, EPI_RELU, ..> with KTW / 2 pairs per wave and tile as the weight source; K = d in one
 *                  chunk of 4, 8 or 16 k-tiles per wave: d = 512 / 1024 / 2048), every result bit-identical to the image launch; a refused
 *                  layer keeps its image launch (vc_debug_read "w8ur_stats": int32 [layer][state, pairs refused]).  10 = 2 + bit 8: also
 *                  at the row counts the measured win table leaves out (for the A/B tool and the tests; vc_debug_w8ur_plan says which row
 *                  counts take the form).  Independent of "w8u", "w8r", "w8m" and "w8w".  One-row steps, passes on the fp32 rows
 *                  ("hq" = 0) and wide steps keep their launches.  The option text gains |w8ur=<v> right behind |w8u=<v> (or where that
 *                  would stand) on such an engine only.  Resident memory: + 0.5 x the W1 image (4 d^2 + d^2 / 128 bytes per layer:
 *                  + 0.27 GB at giga830M) whatever max_seqs is, nothing where "w8u" already holds the planes
 *   "w8q"          0 / 4 / 12, ONLY on an engine that called vc_request_w8_qkv_rows (default 4; VC_EINVAL on any other engine and for any
 *                  other value): the passes of finished rows behind a centred copy (option "hq") whose QKV projection reads the
 *                  12-channel image - the row counts past the paired consumer's: 9..16 at every width, 7 and 8 at d = 2048, and the
 *                  lower ones too with "qkv_p8" below 2 - stream the QKV projection of layers 1.. (4) from the E4M3 pairs of that image
 *                  (csrc/vc_w8.h "w8q": 768 B of codes and two side bytes, one per part, per 12 channels x 64 inputs;
 *                  rows_gemm_qkvq_w8_k: the text of rows_gemm_k<bf16, KTW, PRO_LNQ, EPI_QKV, ..> with KTW / 2 pairs per wave and tile as
 *                  the weight source; K = d in one chunk of 4, 8 or 16 k-tiles per wave: d = 512 / 1024 / 2048), every result
 *                  bit-identical to the image launch; a refused layer keeps its image launch, and so does layer 0, which reads no
 *                  centred copy (vc_debug_read "w8q_stats": int32 [layer][state, pairs refused]).  12 = 4 + bit 8: also at the row
 *                  counts the measured win table leaves out (for the A/B tool and the tests; vc_debug_w8q_plan says which row counts
 *                  take the form).  Independent of "w8r", "w8m", "w8w", "w8u" and "w8ur".  The option text gains |w8q=<v> right behind
 *                  |w8ur=<v> (or where that would stand) on such an engine only.  Resident memory: + 0.5 x the Wqkv image per packed
 *                  layer (3 d^2 + d^2 / 128 bytes: + 0.20 GB at giga830M) whatever max_seqs is
 *   "kv8"          0 / 1, ONLY on an engine that called vc_request_kv8 (default 1; VC_EINVAL on any other engine): decode passes read the
 *                  cached K / V positions older than the pass as one OCP E4M3 byte per value times 2^shift, one shift byte per cached
 *                  row of a head (csrc/vc_kv8.h; voicecraft_amd/quant.py kv8_quantize_rows states the grid), half the bytes of the bf16
 *                  rows; the pass's own rows and every prefill pass stay on the bf16 cache.  One more launch per pass (kv8_pack_k)
 *                  quantises the rows the pass wrote, whatever the option's value.  This CHANGES values: 3 mantissa bits are left of
 *                  a cached value.  The option text ends in |kv8=<v> on such an engine only.  Resident memory: K/V x 1.5 + 2 / head_dim
 *                  An engine that called vc_request_kv8c runs the centred forms of the same launches (K codes of k - c, below).
 * What an option may change: nothing in the exact fp32 mode's greedy tokens (tests/test_gpu_options.py, test_gpu_one_row.py); in bf16
 * mode the forms that re-order sums or round at another place ("finished_rows", "fr_pair", "att_p16", "hq", "fr_one", "qkv_p8", "attn_fast",
 * "qkv16", "wide_heads", "wide_gemm") move head logits by bf16 rounding (tests allow 0.25 absolute), so top-k SAMPLED tokens can differ between option
 * states; the cache-policy / data-path / host-side options ("nt", "wd_stage", "graph_steps", "shrink", "w13", "w8", "w8r", "w8m", "w8w", "w8u", "w8ur", "w8q") change no value; "kv8" rounds cached K / V to its grid.
 * The non-temporal mask "nt" has no bit for the finished-row producers (rows_gemm_fr_k, rows_gemm_fr2_k, row_gemm_fr1_k) and the
 * wide-decode kernels: they always stream with the hint.  Captured decode graphs are kept per option state and step width, so an
 * in-process A/B (bench.py --ab) pays for capture once per state.  Unknown names / malformed values: VC_EINVAL.
 * (Left the tree in round 6: the prefetch roles "attn_pf", "attn_pf_cut", "gemm_pf" - default-off, or inside the spread on the driver's
 * box -, and the knobs "ln_trim", "lnw_tiles", "fr_split_rows", "attn_blocks", "attn_blocks1", "ln_split_rows", "mt_tiles", whose measured
 * best value is a constant now) */
int vc_set_option(vc_engine* e, const char* name, const char* value);

/* ---- weights: replaces get_model()/load_state_dict (inference_tts_scale.py:107-125).
 * `key` is the reference state_dict key; data is fp32 (or int64 for
 * eog/eos, ignored).  `on_device` tells whether `data` is a host or device pointer.
 * Unknown keys (e.g. accuracy_metrics.*) are ignored and return VC_OK. */
int vc_load_tensor(vc_engine* e, const char* key, const void* data, int on_device,
                   int dtype, const int64_t* shape, int ndim);
/* Packs everything into the MFMA fragment layout in `compute_dtype`
 * (VC_DTYPE_BF16, or VC_DTYPE_F32 for the exact mode), builds the sinusoidal
 * position tables (models/modules/embedding.py:69-92) and frees the staging copies. */
int vc_finalize_weights(vc_engine* e, int compute_dtype);
/* Before vc_finalize_weights (VC_ESTATE after it): also pack the matrices of `mask` (1 FFN down-projection, 4 QKV projection; any
 * other bit: VC_EINVAL) of every layer as E4M3 bytes for one-row steps, option "w8" above.  The form is bf16 only: vc_finalize_weights
 * with VC_DTYPE_F32 after a non-zero request returns VC_EINVAL.  An engine without the request packs nothing more and behaves as before. */
int vc_request_w8(vc_engine* e, int mask);
/* After vc_request_w8 on the same engine (VC_ESTATE without it) and before vc_finalize_weights (VC_ESTATE after it): steps of 2..8
 * finished rows stream the requested planes too, option "w8r" above.  `mask`: bits 1 and 4 as above, a subset of vc_request_w8's (anything
 * else: VC_EINVAL).  Nothing more is packed.  An engine without this request has no such option and launches what it launched before. */
int vc_request_w8_rows(vc_engine* e, int mask);
/* After vc_request_w8 on the same engine (VC_ESTATE without it) and before vc_finalize_weights (VC_ESTATE after it): passes of 9..16
 * finished rows stream the FFN-down planes too, option "w8m" above.  `mask`: 1 (FFN-down), a subset of vc_request_w8's (anything else:
 * VC_EINVAL; bit 4, QKV, is refused with a message: no kernel reads the 8-channel QKV image at these row counts).  Nothing more is
 * packed and resident memory does not change.  An engine without this request has no such option and launches what it launched before. */
int vc_request_w8_mid(vc_engine* e, int mask);
/* After vc_request_w8 on the same engine (VC_ESTATE without it) and before vc_finalize_weights (VC_ESTATE after it): steps of 17..64
 * rows stream the matrices of `mask` as E4M3 pair planes, option "w8w" above.  `mask`: bits 1 and 4 as above, a subset of
 * vc_request_w8's (anything else: VC_EINVAL).  vc_finalize_weights then packs the 16-channel images of those matrices once more, for
 * an engine that can run wide steps (max_seqs > 16): + 0.5 x the two images resident, + 0.47 GB at giga830M.  An engine without this
 * request packs nothing more, has no such option and launches what it launched before. */
int vc_request_w8_wide(vc_engine* e, int mask);
/* After vc_request_w8 on the same engine (VC_ESTATE without it) and before vc_finalize_weights (VC_ESTATE after it): steps of 17..64
 * rows stream the FFN up-projection as E4M3 pair planes, option "w8u" above.  `mask`: 2 (anything else: VC_EINVAL); it needs no bit of
 * vc_request_w8's mask and no vc_request_w8_wide.  The weights are taken as given: linear1.weight folded with norm2.weight must lie
 * on the grid (voicecraft_amd/quant.py quantize_state_dict_w8(..., ffn_up=True)), a layer that does not is refused and
 * keeps its image launch.  vc_finalize_weights then packs the 16-channel image W1 once more, for an engine that can run wide steps
 * (max_seqs > 16): + 0.5 x that image resident, + 0.27 GB at giga830M; bf16 only, as vc_request_w8.  An engine without this request
 * packs nothing more, has no such option and launches what it launched before. */
int vc_request_w8_up(vc_engine* e, int mask);
/* After vc_request_w8 on the same engine (VC_ESTATE without it) and before vc_finalize_weights (VC_ESTATE after it): passes of 2..16
 * finished rows stream the FFN up-projection from E4M3 pair planes, option "w8ur" above.  `mask`: 2 (anything else: VC_EINVAL); it needs
 * no bit of vc_request_w8's mask and no other request.  The weights are taken as given, as for vc_request_w8_up: a layer whose folded
 * linear1.weight is off the grid is refused and keeps its image launch.  vc_finalize_weights packs the 16-channel image W1 once more,
 * whatever max_seqs is (once when vc_request_w8_up asked too): + 0.5 x that image resident, + 0.27 GB at giga830M; bf16 only, as
 * vc_request_w8.  An engine without this request packs nothing more, has no such option and launches what it launched before. */
int vc_request_w8_up_rows(vc_engine* e, int mask);
/* After vc_request_w8 on the same engine (VC_ESTATE without it) and before vc_finalize_weights (VC_ESTATE after it): the passes of
 * finished rows whose QKV projection reads the 12-channel image (9..16 rows; 7 and 8 at d = 2048) stream it from E4M3 pairs of that
 * image, option "w8q" above.  `mask`: 4 (anything else: VC_EINVAL); it needs no bit of vc_request_w8's mask and no other request.  The
 * weights are taken as given: a layer whose folded in_proj_weight is off the grid is refused and keeps its image launch.
 * vc_finalize_weights packs the 12-channel image Wqkv of layers 1.. once more, whatever max_seqs is: + 0.5 x that image resident,
 * + 0.20 GB at giga830M; bf16 only, as vc_request_w8.  An engine without this request packs nothing more, has no such option and launches
 * what it launched before. */
int vc_request_w8_qkv_rows(vc_engine* e, int mask);
/* Before vc_finalize_weights (VC_ESTATE after it): keep, next to every layer's bf16 K / V cache, an E4M3 copy (one byte per value) and one
 * shift byte per cached row of a head, written by one packer launch behind every pass, and let the decode attention read the positions
 * older than the pass from it (option "kv8" above).  bf16 only: vc_finalize_weights with VC_DTYPE_F32 after the request returns
 * VC_EINVAL.  An engine without the request allocates and launches nothing more and behaves as before. */
int vc_request_kv8(vc_engine* e);
/* vc_request_kv8 with CENTRED K (the same call order and dtype rules; implies it).  Next to the E4M3 copy the engine keeps, per layer,
 * cache slot and head, a bf16 centre c[head_dim] - the mean K row of the prefill pass that wrote the slot's position 0 (csrc/vc_kv8.h
 * states the contract; voicecraft_amd/quant.py kv8c_* restates it) - found by one more launch in front of the packer on prefill passes
 * (kv8c_centre_k).  K codes stand for k - c, the decode attention adds q . c to every 8-bit score: softmax does not see the common
 * offset of the K rows, which is where the plain grid loses its bits on peaked attention.  V is as in the plain mode.
 * Option "kv8" keeps its 0 / 1 meaning; the option text ends in |kv8c=1 on such an engine only (there is no option "kv8c").  vc_debug_read: "kcentre_<l>" bf16
 * [max_seqs][H][head_dim], "kcentre_rows" int32 [max_seqs] (n0 per slot).  Resident memory: + max_seqs x d_model x 2 bytes per layer. */
int vc_request_kv8c(vc_engine* e);

/* ---- TTS: VoiceCraft.inference_tts (models/voicecraft.py:908-1153) and, with
 * n_samples > 1, VoiceCraft.inference_tts_batch (:1156-1439, best-of-N: the sample
 * whose first codebook terminates first is kept).
 *   x_dev      int64 [Lx]            phoneme ids
 *   y_dev      int64 [T][K]          prompt codes, time-major exactly as the caller's y[0]
 *   forced_dev int64 [n_forced][B][K] optional teacher-forcing trajectory (parity hook, see
 *                                    vc_sample_cfg.forced_mode; B = n_samples); NULL = sample
 *   res_dev    int64 [K][res_cap]    out: prompt followed by generated frames (row stride res_cap)
 *   gen_len    out (host): number of generated frames Tg; res holds T+Tg columns
 *   logits_dev float [logit_steps][B][K][V] optional: raw head outputs of the first steps
 *   n_steps    out (host, optional): decode steps taken (Tg + K)                       */
int vc_tts(vc_engine* e, const int64_t* x_dev, int Lx, const int64_t* y_dev, int T,
           const vc_sample_cfg* sc, int n_samples, const int64_t* forced_dev, int n_forced,
           int64_t* res_dev, int res_cap, int* gen_len, float* logits_dev, int logit_steps,
           int* n_steps, void* stream);

/* ---- streaming TTS: vc_tts for ONE utterance and one sample (inference_tts semantics), resumable - the generated frames are
 * handed out while the decode loop runs instead of after its last step.  The loop is the blocking call's: the same captured graphs,
 * at most two graph batches queued, the host pacing one batch behind the device; after each pacing wait the host knows that
 * `graph_steps` more steps are complete and that their rows of the generated-token buffer are final (overrides happen at sampling
 * time, nothing rewrites a row).  The delay pattern makes frame t complete once step t + K - 1 has run, so after S finished steps
 * of a live sequence frames < S - (K - 1) are complete; once the sequence has ended the count is its own Tg.  Same tokens, same
 * number of launched steps, same Philox stream as vc_tts with the same arguments.
 * Not streamable, and refused: best-of-N (n_samples > 1: the kept sample is unknown until a group terminates), the multi-utterance
 * calls and editing - they have no stream form.
 *   begin  does what vc_tts does up to and including the first sample (graphs pre-captured ahead of the timers, prompt, prefill,
 *          state upload, first sample).  x_dev / y_dev / forced_dev must stay valid until end.  forced_dev: as in vc_tts (B = 1).
 *   next   queues and paces graph batches exactly as the blocking loop does and returns as soon as at least min_frames new frames
 *          are complete, or the sequence has ended: frames [first_frame, first_frame + n_frames) un-shifted into codes_dev
 *          [K][cap] (row stride cap, time-major like res; n_frames <= cap; 1 <= min_frames <= cap).  *done = 1 once every frame
 *          has been handed out (possibly with n_frames = 0).  The gather runs on a side stream the engine owns and only that
 *          stream is synchronised: the decode stream gets no synchronisation inside the loop.
 *   end    drains the loop if frames are still outstanding, assembles the full result exactly as vc_tts does (res_dev, res_cap,
 *          gen_len, n_steps as there) and fills vc_last_timing.  res_dev = NULL aborts: what is queued is waited for, nothing is
 *          assembled, the engine is reusable.  Either way the stream is closed.
 * While a stream is open every other decode entry point, vc_set_option and a second begin return VC_ESTATE; next / end without
 * an open stream return VC_ESTATE; bad pointers, cap < 1, min_frames < 1 or > cap return VC_EINVAL (checked first).  An error
 * returned by next leaves the stream open: close it with end (res_dev = NULL, or a buffer to get the same error once more). */
int vc_tts_stream_begin(vc_engine* e, const int64_t* x_dev, int Lx, const int64_t* y_dev, int T,
                        const vc_sample_cfg* sc, const int64_t* forced_dev, int n_forced, void* stream);
int vc_tts_stream_next(vc_engine* e, int min_frames, int64_t* codes_dev, int cap,
                       int* first_frame, int* n_frames, int* done);
int vc_tts_stream_end(vc_engine* e, int64_t* res_dev, int res_cap, int* gen_len, int* n_steps);

/* ---- decode sessions: continuous batching of TTS and speech-editing requests (inference_tts / inference semantics; a TTS request may
 * be best-of-N, inference_tts_batch semantics, in a session opened for it).
 * A session keeps the decode loop open: requests are submitted at any time, each is prefilled into a free K/V slot between two graph
 * batches and joins the running batch, and each result can be fetched as soon as its own sequence has ended - the batch is refilled
 * instead of idling to its longest member.  The step width follows the live count both ways (the next power of two, captured graphs
 * per width).  Both kinds of request share one decode step: an editing request decodes one row per step with its span switches fed
 * over three steps, as in vc_edit_multi.
 * Sampling controls: top_k, top_p, temperature and stop_repetition are per REQUEST (vc_request_ctl; NULL = the values given at open);
 * silence_tokens and use_graph are the session's, fixed at open.  The seed is per request: a request draws on the Philox stream (its
 * seed, sequence 0, its own step, codebook) - the stream of a lone vc_tts / vc_edit_multi call with that seed - whatever slot it lands
 * in.  Exact mode: every request's tokens are those of its own blocking call with its controls, whatever it shared a step with.  bf16:
 * the tokens are a function of the submissions and of the turn each was made at (the admission schedule is decided from retirements of
 * batches the host has seen end, never from how far the device runs ahead).
 * Best-of-N requests: a session opened with vc_session_open_best_of(max_samples > 1) takes TTS requests of n_samples in [1, max_samples]
 * samples (vc_session_submit_best_of).  One ticket, N slots and N rows: the prompt is prefilled once and its K/V replicated to the N - 1
 * sibling slots; sample j draws on (the request's seed, sequence j, its own step, codebook), the stream of a lone vc_tts(n_samples = N)
 * call; the LAST sample whose first codebook terminates first is kept, the others are dropped at that step and their rows and slots
 * return to the session.  The steps of such a session end in two sampler launches instead of one (the keep decision reads every
 * member's terminator flag, which needs a kernel boundary); a session opened with vc_session_open runs the one-launch steps.  Exact
 * mode: tokens and kept index are those of the request's own vc_tts(n_samples = N) call.  bf16: a function of the submission schedule,
 * but not bit-equal to the blocking call (the session narrows after a group collapses, the blocking one-group call keeps its N rows).
 * Not part of a session, because they have no per-request form here: a shared text prefix, logits_out and forced trajectories - the
 * entry points below simply have no such arguments; use the blocking calls.  Editing and best-of-N tickets do not stream (frames).
 *   open     max_live in [1, max_seqs] slots.  Captures the step graphs of every width the session can pass through (the powers of two
 *            up to the one for max_live), ahead of any timer.  VC_ESTATE while a streaming call or another session is open.  While a
 *            session is open every other decode entry point, vc_set_option and vc_tts_stream_begin return VC_ESTATE.
 *   open_best_of  the same with max_samples in [1, max_live] (VC_EINVAL outside): the largest n_samples a request may ask for.
 *            max_samples = 1 is exactly vc_session_open.
 *   submit   a TTS request with the session's controls (submit_ctl with ctl = NULL).  submit_ctl: a TTS request with its own controls.
 *            Host-side checks at once, with vc_tts's codes: empty text (VC_EINVAL), a prompt that alone does not fit max_positions
 *            (VC_ECAP); a ctl whose temperature is not a finite positive number or whose top_p is not a number: VC_EINVAL.  The
 *            request joins a FIFO; *ticket identifies it.  x_dev / y_dev must stay valid until the ticket is fetched or the session
 *            closed; ctl is copied.
 *   submit_best_of  a TTS request of n_samples samples (n_samples = 1 is submit_ctl).  n_samples outside [1, max_samples] of the session:
 *            VC_EINVAL naming both numbers, and the session goes on.  The request takes n_samples free slots - the lowest free ones,
 *            not necessarily consecutive - and is admitted by the first turn that has them; admission stays strictly FIFO, so nothing
 *            submitted behind it is admitted before it (head-of-line blocking).  Editing requests have no best-of-N form.
 *   submit_edit  an editing request: mask_intervals [M][2] and mask_values [2M] are host arrays with vc_edit's meaning, copied at
 *            submit.  Validated at once with vc_edit's codes and messages (span count; ordered, disjoint intervals; an empty non-masked
 *            piece; mask value range; eos > 0 without reduced_eog; the rearranged prompt against max_positions and the prefill arena).
 *            A refused submit of any kind leaves the session running.
 *   advance  one turn: wait for the older of the two batches in flight; note what it (or an earlier one) retired; admit from the FIFO
 *            into the free slots, in order; queue the prefill of the admitted requests (both kinds in one pass), the re-pack to the
 *            width now needed, their first sample and the next batch.  tickets_out[0 .. *n_finished) = the requests found finished this
 *            turn, at most cap of them: one there is no room for is reported by a later turn (and holds its slot until then), so cap >=
 *            max_live reports every request in the turn that finds it.  If the queued work of a turn fails after requests were
 *            admitted, the session is broken: this and every later submit / advance return the error (VC_ESTATE afterwards) until it
 *            is closed.  *idle = 1 when nothing is live, pending or in flight: an idle session queues nothing, and a later submit
 *            restarts it.
 *   fetch    assembles a finished request and frees its slot; res_dev = NULL drops it.  A TTS ticket: exactly as vc_tts does (res_dev
 *            [K][res_cap], *gen_len = the generated frames Tg, res holds T + Tg columns).  An edit ticket: exactly as vc_edit does
 *            (nonmask_0, gen_0, ..., nonmask_M) and *gen_len receives the RESULT length T'.  *n_steps = the request's own sampled
 *            steps (the fed rows of a span switch are not steps).  Unknown ticket: VC_EINVAL; unfinished: VC_ESTATE; ran out of
 *            positions before its terminator (an edit: before its last span ended): VC_ECAP, as vc_tts / vc_edit_multi; an
 *            out-of-range token id in its x / y: VC_EINVAL naming the ticket.  A finished request holds its slot until fetched (the
 *            slot's rows of the generated-token log are the result).  A best-of-N ticket is finished by the turn that has seen all its
 *            samples retire; a dropped sample's slot is free as soon as the host has seen its batch end, only the kept sample's slot is
 *            held for the fetch, which assembles from it.  No sample terminated within its room: VC_ECAP "no sample terminated within
 *            the step budget", as vc_tts_multi_best_of.
 *   kept     *kept = the kept sample's index of a finished, unfetched best-of-N ticket (-1: none terminated); 0 for any other ticket.
 *            Unknown ticket: VC_EINVAL; unfinished: VC_ESTATE.
 *   stats    (requests in [0], [1]; every sample's rows in [5], [6])  [0] requests admitted, [1] of them admitted while other sequences were live, [2] turns, [3] widenings, [4] narrowings,
 *            [5] sum over launched steps of the rows that were live, an edit's fed rows included (counted at retirement), [6] sum over
 *            launched steps of the step width, [7] microseconds of decode-stream time spent on admissions (prefill + re-pack + first
 *            sample; HIP events).
 *   frames   the frames of live TTS tickets while they decode (streaming): for each of the n tickets, frames [first_frame[i],
 *            first_frame[i] + n_frames[i]) un-shifted into block i of codes_dev [n][K][cap] (row stride cap, as vc_tts_stream_next
 *            lays them out: out[j][t] = the log's row t + j, codebook j).  The call never advances the loop, queues nothing on the
 *            decode stream and waits for nothing on it: it hands out what the host already knows to be final.  A request admitted by
 *            the turn that queued batch b has 1 + graph_steps * (known - b + 1) final rows once advance has seen batch known >= b end
 *            (none before), and its own frame count - the gen_len fetch reports - once its retirement is among the ended batches,
 *            whether or not advance has reported it yet; frame t needs rows t .. t + K - 1.  What is handed out when is therefore a
 *            function of the submission schedule, like the admissions.  A ticket gets frames only when at least min_frames are
 *            ready, or, once it has ended, all the rest however few (never more than cap per call); done[i] = 1 once it has ended
 *            and every frame has been handed out.  A pending ticket: 0 frames, done 0.  A ticket that ended without a result (ran out
 *            of positions; an out-of-range token id, of which no frame is ever handed out): done 1 and no further frames - fetch
 *            still reports the error.  A finished ticket streams until it is fetched.  The gather is one launch for all tickets on
 *            the side stream of vc_tts_stream_next, and only that stream is synchronised.  Refused as a whole, before any cursor
 *            moves, with VC_EINVAL: an unknown or fetched ticket, a ticket given twice, an editing ticket ("editing requests do not
 *            stream": its rows per batch hang on span switches the host learns at retirement, and its result is a splice), a best-of-N
 *            ticket ("best-of-N requests do not stream": the kept sample is unknown until the group decides), n outside
 *            [1, max_live], cap < 1, min_frames outside [1, cap], null pointers.  No session: VC_ESTATE; a broken session: its error.
 *   cancel   takes one request out of the session, in whatever state it is; *was (may be NULL) = the state it was in: 0 pending, 1 live,
 *            2 finished and not yet fetched.  The call never waits for the device and queues nothing.  From it on the ticket is gone:
 *            advance never reports it, and fetch / kept / frames / cancel refuse it as an unknown ticket.  No partial result comes
 *            back (stream the request to have its frames; frames already handed out stay valid, a prefix of what it would have made).
 *            Pending: it leaves the FIFO at once, the order of the others unchanged, and its x_dev / y_dev are never read; if it was
 *            blocking the head of the line the next advance admits whatever now fits.  Finished: exactly fetch(res_dev = NULL), the
 *            slot is free at once (so is a request that has retired in a batch advance has seen end but could not report, tickets_out
 *            being full).  Live: the next advance retires every row of the ticket that has not retired yet (a TTS or editing
 *            request's one row, an edit in the middle of a span switch included; every remaining member of a best-of-N group) in one
 *            launch for all cancels made since the last turn, in front of its re-pack.  The slots come back the way any retired row's
 *            do - when advance has seen the batch end that the retirement is stamped with: a cancel made before the turn that queues
 *            batch c frees its slots in the turn that queues batch c + 2, that is 2 * graph_steps steps later, so admissions, widths
 *            and bf16 tokens stay a function of the schedule of submissions AND cancels.  A ticket found finished by the same advance
 *            that applies its cancel is dropped, not reported.  Cancelling every live request leads to *idle = 1 as usual.  The
 *            x_dev / y_dev of a cancelled LIVE ticket may still be read by the prefill queued by the turn that admitted it: they must
 *            stay valid until the second advance after the cancel has returned, or until the session is closed.  A cancelled request
 *            that had been admitted stays counted in stats [0], and the rows it really ran in [5].  Unknown ticket, or one fetched or
 *            cancelled already: VC_EINVAL naming the ticket, and the session goes on.  No session: VC_ESTATE; a broken session: its
 *            error.
 *   close    waits for what is queued, drops everything pending and unfetched; the engine is reusable. */
typedef struct vc_request_ctl {   /* 16 bytes: the per-request part of vc_sample_cfg, same meaning field by field */
  int32_t top_k;
  float top_p;
  float temperature;
  int32_t stop_repetition;
} vc_request_ctl;
int vc_session_open(vc_engine* e, int max_live, const vc_sample_cfg* sc, void* stream);
int vc_session_open_best_of(vc_engine* e, int max_live, int max_samples, const vc_sample_cfg* sc, void* stream);
int vc_session_submit(vc_engine* e, const int64_t* x_dev, int Lx, const int64_t* y_dev, int T, uint64_t seed, int* ticket);
int vc_session_submit_ctl(vc_engine* e, const int64_t* x_dev, int Lx, const int64_t* y_dev, int T,
                          const vc_request_ctl* ctl, uint64_t seed, int* ticket);
int vc_session_submit_best_of(vc_engine* e, const int64_t* x_dev, int Lx, const int64_t* y_dev, int T, int n_samples,
                              const vc_request_ctl* ctl, uint64_t seed, int* ticket);
int vc_session_submit_edit(vc_engine* e, const int64_t* x_dev, int Lx, const int64_t* y_dev, int T,
                           const int32_t* mask_intervals, int M, const int32_t* mask_values,
                           const vc_request_ctl* ctl, uint64_t seed, int* ticket);
int vc_session_advance(vc_engine* e, int* tickets_out, int cap, int* n_finished, int* idle);
int vc_session_fetch(vc_engine* e, int ticket, int64_t* res_dev, int res_cap, int* gen_len, int* n_steps);
int vc_session_kept(vc_engine* e, int ticket, int* kept);
int vc_session_frames(vc_engine* e, int n, const int* tickets, int min_frames, int64_t* codes_dev, int cap,
                      int* first_frame, int* n_frames, int* done);
int vc_session_cancel(vc_engine* e, int ticket, int* was);
int vc_session_stats(vc_engine* e, int64_t out[8]);
int vc_session_close(vc_engine* e);

/* ---- multi-utterance TTS (SURVEY.md §8f-1 / BASELINE config 5): B independent
 * (x, y) pairs decoded as one batch; each row follows inference_tts exactly.
 *   x_dev int64 [sum Lx], y_dev int64 [sum T][K] concatenated; *_off host arrays [B+1].
 *   res_dev int64 [B][K][res_cap]; gen_len host [B].
 *   forced_dev / logits_dev: as in vc_tts, indexed by each sequence's own step count.
 *   shared_text_prefix: the first P text tokens are IDENTICAL in every sequence (the sentence-chained
 *     "Long TTS" of gradio_app.py:231-236, :249-313: every sentence is synthesised as
 *     [transcript of the voice prompt ; sentence] against the same audio prompt).  Text precedes audio in the
 *     sequence and attention is causal, so the K/V of those P positions do not depend on what follows: they
 *     are computed once (sequence 0) and every sequence's attention reads them there - exact, no copy.
 *     (The audio prompt's K/V DO depend on the whole text and cannot be shared.)  0 = nothing shared;
 *     the equality is verified on the device while the prompts are built: a text that differs from sequence 0's
 *     inside the prefix makes the call fail with VC_EINVAL before anything is decoded. */
int vc_tts_multi(vc_engine* e, int B, const int64_t* x_dev, const int32_t* x_off,
                 const int64_t* y_dev, const int32_t* y_off, const vc_sample_cfg* sc,
                 int shared_text_prefix,
                 const int64_t* forced_dev, int n_forced, int64_t* res_dev, int res_cap, int* gen_len,
                 float* logits_dev, int logit_steps, int* n_steps, void* stream);

/* ---- multi-utterance best-of-N TTS: B utterances x n_samples (N) samples as B*N sequences - every sentence of the reference's
 * "Long TTS" goes through inference_tts_batch(batch_size = sample_batch_size) (gradio_app.py:249-280, inference_tts_scale.py:61-87),
 * here all of them in one call.  Sample j of utterance u is the sequence of slot u*N + j and a member of best-of-N group u; each
 * utterance behaves exactly like vc_tts(..., n_samples = N) on its own prompt (the LAST sample whose first codebook terminates
 * first is kept, models/voicecraft.py:1296-1302).  vc_tts is the case (1, N) of this call and vc_tts_multi the case (B, 1).
 *   x_dev / x_off / y_dev / y_off / shared_text_prefix: as vc_tts_multi (positions below the prefix are read from slot 0)
 *   res_dev int64 [B][K][res_cap]; gen_len host [B]; kept host [B] (may be NULL): the sample index 0..N-1 each utterance kept
 *   forced_dev int64 [n_forced][B*N][K], logits_dev float [logit_steps][B*N][K][V]: utterance-major, indexed by slot
 *   The Philox stream is keyed by slot (vc_sample_cfg.seed), so utterance 0's draws are the draws of a lone vc_tts call with the
 *   same seed; utterance u > 0 draws on the streams of slots u*N .. u*N + N-1.
 *   B*N > max_seqs: VC_ECAP; n_samples < 1: VC_EINVAL; an utterance none of whose samples terminated within the step budget:
 *   VC_ECAP ("utterance 3: ..."). */
int vc_tts_multi_best_of(vc_engine* e, int B, int n_samples, const int64_t* x_dev, const int32_t* x_off,
                         const int64_t* y_dev, const int32_t* y_off, const vc_sample_cfg* sc, int shared_text_prefix,
                         const int64_t* forced_dev, int n_forced, int64_t* res_dev, int res_cap, int* gen_len,
                         int* kept, float* logits_dev, int logit_steps, int* n_steps, void* stream);

/* ---- speech editing: VoiceCraft.inference (models/voicecraft.py:561-906).
 *   mask_intervals host int32 [M][2] (codec-frame units, as mask_interval[0])
 *   mask_values    host int32 [2M]   the reference's mask_value list (insert_mask, :264-288)
 *   res_dev int64 [K][res_cap]; res_len out (host): T' (voicecraft.py:900)            */
int vc_edit(vc_engine* e, const int64_t* x_dev, int Lx, const int64_t* y_dev, int T,
            const int32_t* mask_intervals, int M, const int32_t* mask_values,
            const vc_sample_cfg* sc, const int64_t* forced_dev, int n_forced,
            int64_t* res_dev, int res_cap, int* res_len, float* logits_dev, int logit_steps,
            int* n_steps, void* stream);

/* ---- batched speech editing: B independent inference requests (each with its own text, audio and 1..max_n_spans
 * spans) decoded as one batch; each request follows vc_edit exactly.  One prefill over all prompts, then ONE decode row
 * per request: a span switch is fed over three one-row steps instead of vc_edit's 3-row step, so the step stays B rows
 * wide and shrinks as requests retire (option "shrink").  Sampling config shared by the whole call.
 *   x_dev int64 [sum Lx], y_dev int64 [sum T][K] concatenated; x_off / y_off host int32 [B+1] (as vc_tts_multi)
 *   mask_intervals host int32 [sum M_i][2], span_off host int32 [B+1]; request i's 2*M_i mask values start at
 *     mask_values + 2*span_off[i] (as vc_eval_forward's spans)
 *   res_dev int64 [B][K][res_cap]; res_len host [B]
 *   forced_dev / logits_dev: [step][B][K](...), indexed by each request's own sampled steps (feed steps are not steps)
 *   B > max_seqs: VC_ECAP.  A request's bad input fails the call with a message naming the request ("request 2: ..."). */
int vc_edit_multi(vc_engine* e, int B, const int64_t* x_dev, const int32_t* x_off,
                  const int64_t* y_dev, const int32_t* y_off,
                  const int32_t* mask_intervals, const int32_t* span_off, const int32_t* mask_values,
                  const vc_sample_cfg* sc, const int64_t* forced_dev, int n_forced,
                  int64_t* res_dev, int res_cap, int* res_len, float* logits_dev, int logit_steps,
                  int* n_steps, void* stream);

/* ---- the training objective, teacher-forced: VoiceCraft.forward (models/voicecraft.py:472-559) for B utterances
 * whose mask intervals are GIVEN (the reference draws them at random, :198-237): rearrange / delay-shift / mask
 * placeholders (:239-320), one non-cached decoder pass over [text ; rearranged audio] of every utterance (:501-512;
 * the reference pads the batch and masks the padding, the engine runs the rows unpadded), the K heads on every audio
 * position (:516), the placeholders dropped and the delay pattern reverted per piece (:374-404,
 * codebooks_patterns.py:247-266), then per codebook the cross-entropy SUM and the number of targets among the ten
 * largest logits (torchmetrics MulticlassAccuracy(top_k=10), :187-195, :540-541).
 *   x_dev int64 (all texts back to back), x_off host int32 [B+1]; y_dev int64 [frames][K] time-major (all utterances
 *   back to back), y_off host int32 [B+1] in frames
 *   spans host int32 [sum M_i][2] frame intervals, span_off host int32 [B+1]; mask_values host int32 [sum M_i]
 *   (the utterance's emb_inds_use, :270-273)
 *   out (host): nll_sum double [K] = sum of -log softmax(logits)[target]; hits int64 [K]; n_targets int64 (per codebook)
 *   nll_dev optional device float [nll_cap][K]: the per-row terms in the engine's row order (parity hook), with
 *   tgt_dev int32 [nll_cap][K] (>= 0 index into y_dev, -1 none, <= -2 constant token -(v+2)); n_rows_out = rows written.
 *   With the hook the engine also keeps the head logits of every row of the call, fp32 [rows][K][V] in the same row order
 *   (vc_debug_read "eval_logits"; a device buffer allocated by the first such call).  Without it nothing is allocated or copied. */
int vc_eval_forward(vc_engine* e, int B, const int64_t* x_dev, const int32_t* x_off,
                    const int64_t* y_dev, const int32_t* y_off,
                    const int32_t* spans, const int32_t* span_off, const int32_t* mask_values,
                    double* nll_sum, int64_t* hits, int64_t* n_targets,
                    float* nll_dev, int32_t* tgt_dev, int64_t nll_cap, int64_t* n_rows_out, void* stream);

/* Host-only half of vc_eval_forward for ONE utterance (no engine, no GPU: checked against the oracle in the CPU tests):
 * the segment table of its training sequence, seg_out int32 [n_seg][6] = {first column, columns, first source frame,
 * source frames, appended terminator or -1, mask_embedding row or -1}, the number of audio columns, and the target
 * table tgt_out int32 [Lx + n_cols][K] as described above (y_frame_off = the utterance's first frame inside y_dev). */
int vc_eval_layout(const vc_model_cfg* cfg, int Lx, int T, const int32_t* spans, int M, const int32_t* mask_values,
                   int y_frame_off, int32_t* seg_out, int* n_seg, int* n_cols, int32_t* tgt_out, int64_t tgt_cap);

/* ---- delayed-codebook pattern (models/codebooks_patterns.py:151-176, :222-245 and
 * the un-shift at models/voicecraft.py:1125-1139).  Integer, bit-exact.  No engine needed.
 *   shift : z [B][K][T]  -> out [B][K][T+K]   out[q][s] = z[q][s-1-q] or `special`
 *   revert: s [B][K][S]  -> out [B][K][T]     out[q][t] = s[q][t+1+q] if t+1+q < S else `special`
 *   unshift: span [N][K] (step-major) -> out [K][N-K]  out[j][t] = span[j+t][j]         */
int vc_pattern_shift(const int64_t* z_dev, int B, int K, int T, int64_t special,
                     int64_t* out_dev, void* stream);
int vc_pattern_revert(const int64_t* s_dev, int B, int K, int S, int T, int64_t special,
                      int64_t* out_dev, void* stream);
int vc_pattern_unshift(const int64_t* span_dev, int N, int K, int64_t* out_dev, void* stream);

/* ---- parity/debug hooks (tests only) ------------------------------------ */
/* n_draws independent draws from one logits row [V] through the product sampler (temperature, top-k,
 * top-p, inverse-CDF on a Philox stream; models/voicecraft.py:26-86): out_dev int32 [n_draws].
 * Only top_k / top_p / temperature / seed of `sc` are read.  No engine needed. */
int vc_debug_sample(const float* logits_dev, int V, const vc_sample_cfg* sc, int n_draws,
                    int32_t* out_dev, void* stream);
/* ONE launch of the decode attention kernel (rows_attn_k, the kernel every decode pass runs) on caller-owned device buffers, through
 * the launcher the engine itself uses.  No engine needed.  Row r attends to cache positions 0..row_pos[r] of sequence row_seq[r];
 * positions below *share_len are read from sequence 0; scale = 1/sqrt(hd).
 *   q fp32 [rows][H*hd]; kcache / vcache [n_seqs][H][S_max][hd] in `dtype` (VC_DTYPE_F32 or VC_DTYPE_BF16), 16-byte aligned like q;
 *   row_seq, row_pos int32 [rows]; n_active, share_len one int32 each (*n_active == 0: every row leaves an empty partial).
 *   Split form (x_out null): att_o [rows][H][nsplit][hd] un-normalised partials (fp32; bf16 when part16), att_ml fp32
 *   [rows][H][nsplit][2] = (running maximum in natural units, sum); an empty split leaves (-inf, 0) and zeros.
 *   Unsplit form (x_out set, nsplit 1): x_out [rows][H*hd] normalised rows in `dtype` (0 for a row with nothing to attend to);
 *   att_o / att_ml are not touched and may be null.
 *   nt / fast / part16: the kernel form, as AttnArgs (non-temporal K/V requests; wave maximum before the exponentials; bf16 partials).
 * VC_EINVAL for what no decode pass can issue: hd not 32 / 64 / 128, nsplit outside 1..8, x_out with nsplit != 1, part16 without
 * bf16 or with x_out, a null or misaligned pointer, rows / H / S_max < 1, a dtype other than the two. */
typedef struct vc_debug_attn_args {
  const float* q;
  const void* kcache;
  const void* vcache;
  const int32_t* row_seq;
  const int32_t* row_pos;
  const int32_t* n_active;
  const int32_t* share_len;
  void* att_o;
  float* att_ml;
  void* x_out;
  int32_t dtype, H, hd, S_max, rows, nsplit, nt, fast, part16;
} vc_debug_attn_args;
int vc_debug_attn(const vc_debug_attn_args* a, void* stream);
/* ONE launch of a prefill attention kernel on caller-owned device buffers, through the launchers the engine itself uses
 * (form 1: tile_attn_k, 16 query rows per workgroup; form 2: tile_attn64_k, 64 query rows per workgroup, bf16 and hd 128 only).
 * No engine needed.  The rows are a prefill pass's: prompts back to back, each starting on a multiple of 16 rows (form 2: 64), the
 * rows of a prompt at consecutive positions of ONE sequence, padding rows (row_pos = -1) only behind a prompt's last row.  Row r
 * attends to cache positions 0..row_pos[r] of sequence row_seq[r]; positions below *share_len are read from sequence 0;
 * scale = 1/sqrt(hd).  The kernels trust the tables: row_seq < n_seqs and row_pos < S_max are the caller's to keep.
 *   q fp32 [rows][H*hd]; kcache / vcache [n_seqs][H][S_max][hd] in `dtype` (VC_DTYPE_F32 or VC_DTYPE_BF16); row_seq, row_pos int32
 *   [rows]; share_len one int32; x_out [rows][H*hd] normalised rows in `dtype`, exact zeros in padding rows; q, the caches and x_out
 *   16-byte aligned.
 * VC_EINVAL, before the device is touched, for what no prefill pass can issue: hd not 32 / 64 / 128, a form other than 1 / 2, form 2
 * without bf16 and hd 128, rows not a positive multiple of 16 (form 2: 64), a null or misaligned pointer, H / S_max < 1, a dtype
 * other than the two. */
typedef struct vc_debug_tile_attn_args {
  const float* q;
  const void* kcache;
  const void* vcache;
  const int32_t* row_seq;
  const int32_t* row_pos;
  const int32_t* share_len;
  void* x_out;
  int32_t dtype, H, hd, S_max, rows, form;
} vc_debug_tile_attn_args;
int vc_debug_tile_attn(const vc_debug_tile_attn_args* a, void* stream);
/* vc_debug_attn for option "kv8" (bf16 only; no engine needed).  base: as above; kcache8 / vcache8: uint8 [n_seqs][H][S_max][hd], one OCP
 * E4M3 code byte per value, 16-byte aligned; kvshift8: int8 [n_seqs][H][S_max][2], the shift of the K row and of the V row.
 *   pack = 1: ONE launch of the packer (kv8_pack_k): the rows (row_seq[r], row_pos[r]) of the bf16 caches are quantised into the three
 *     arrays (pos < 0: none; *n_active == 0: nothing at all); every other byte stays.  q, share_len, the outputs, nsplit and the form
 *     flags are not read.
 *   pack = 0: ONE launch of rows_attn_k in its kv8 form.  The rows are `rps` consecutive rows per sequence at consecutive positions; row r
 *     reads the positions below lo = row_pos[r - r % rps] from the E4M3 arrays (times 2^shift) and lo..row_pos[r] from the bf16 caches.
 * VC_EINVAL, before the device is touched: what vc_debug_attn refuses, a dtype other than bf16, rps < 1, a null or misaligned array. */
typedef struct vc_debug_attn8_args {
  vc_debug_attn_args base;
  void* kcache8;
  void* vcache8;
  void* kvshift8;
  int32_t rps, pack;
} vc_debug_attn8_args;
int vc_debug_attn8(const vc_debug_attn8_args* a, void* stream);
/* vc_debug_attn8 for the centred mode (vc_request_kv8c; no engine needed).  centre: bf16 [n_seqs][H][hd], 16-byte aligned.
 *   mode = 0: ONE launch of rows_attn_k in its centred kv8 form: as vc_debug_attn8's pack = 0, and every score of a position read from the E4M3
 *     arrays gains q . centre[row_seq[r]][h].
 *   mode = 1: ONE launch of the centred packer: as vc_debug_attn8's pack = 1, the K codes and shifts being those of bf16_rne(k - centre[seq][h]);
 *     the V half is the plain one.  (base8.pack is not read.)
 *   mode = 2: ONE launch of the centre kernel over the rows (row_seq, row_pos) as a PREFILL pass's: for every slot < n_seqs whose position 0
 *     is among the rows, centre[slot] = the mean of its K rows in the pass (bf16 kcache; fp32 sums, rounded to bf16) and n0[slot] = their
 *     number; while *share_len > 0 every slot with a row in the pass takes sequence 0's.  Everything else stays.  Only kcache, the row
 *     tables, n_active and share_len of the base are read.
 * VC_EINVAL, before the device is touched: what vc_debug_attn8 refuses, a mode outside 0..2, a null or misaligned centre; mode 2: a null
 * n0, n_seqs outside 1..64, more than 2048 rows. */
typedef struct vc_debug_attn8c_args {
  vc_debug_attn8_args base8;
  void* centre;
  void* n0;          /* int32 [n_seqs], mode 2 */
  int32_t mode, n_seqs;
} vc_debug_attn8c_args;
int vc_debug_attn8c(const vc_debug_attn8c_args* a, void* stream);
/* Host only: what the kv8 options add to a pass - the function the engine's passes follow.  request: 0 none, 1 vc_request_kv8,
 * 2 vc_request_kv8c; kv8: the option's value; rps: rows per sequence of a decode pass, 0 = a prefill pass; rows_attn: the pass's
 * attention is rows_attn_k.  out[0] = the form of the attention launches (VC_KV8_ATTN_*), out[1] = the number of launches queued behind
 * the last layer, out[2], out[3] = those launches in order (VC_KV8_LAUNCH_*, 0 = none).  VC_EINVAL: a request outside 0..2, rps < 0. */
#define VC_KV8_ATTN_PLAIN 0
#define VC_KV8_ATTN_E4M3 1
#define VC_KV8_ATTN_CENTRED 2
#define VC_KV8_LAUNCH_CENTRE 1
#define VC_KV8_LAUNCH_PACK 2
#define VC_KV8_LAUNCH_PACK_CENTRED 3
int vc_debug_kv8_plan(int request, int kv8, int rps, int rows_attn, int32_t out[4]);
/* Host only: the kv8 quantiser (csrc/vc_kv8.h, the code the packer runs) on n_rows rows of hd bf16 values: codes uint8 [n_rows][hd],
 * shift int8 [n_rows].  The CPU tests hold it against voicecraft_amd/quant.py kv8_quantize_rows. */
int vc_kv8_quantize_host(const uint16_t* bf16_rows, int n_rows, int hd, uint8_t* codes, int8_t* shift);
/* Host only: the centred quantiser (csrc/vc_kv8.h vc_kv8c_quantize_row) on n_rows K rows of hd bf16 values against ONE centre of hd bf16
 * values.  The CPU tests hold it against voicecraft_amd/quant.py kv8c_quantize_rows. */
int vc_kv8c_quantize_host(const uint16_t* bf16_rows, const uint16_t* centre, int n_rows, int hd, uint8_t* codes, int8_t* shift);
/* Diagnosis of the BOX, not of the model (no engine needed): ONE thread walks `hops` dependent loads over a ring of `bytes` bytes and
 * stamps the per-XCD shader clock and the chip-wide 100 MHz counter around the walk.  res[0] = ns per dependent load as a lone
 * workgroup on an otherwise idle chip sees it, res[1] = the shader clock (MHz) that workgroup really ran at.  The one-sequence
 * sampler launch is exactly such a workgroup; bench.py prints both numbers (`box`) next to the sampler's time. */
int vc_box_probe(long long bytes, int hops, float res[2], void* stream);
/* Host-only (no engine, no GPU): how a decode pass of `rows` rows is launched for this model shape and compute dtype.
 * out[0] rows up to which the finished-row form applies; out[1] form of this pass (0 slabs + rows-GEMM, 1 finished rows, 2 wide
 * decode); out[2] attention splits; out[3] consumer kernel shape (GemmArgs.mt) or -1; out[4] / out[5] producer form of the
 * out-projection / FFN down-projection (1 one piece, 2 K in two halves, 0 = NOT LAUNCHABLE, -1 n/a); out[6] heads-1 folds finished
 * rows itself; out[7] the consumers' tile counts are even.
 * The default forms of rounds 5-6 (-1 where the row count does not take them): out[8] ONE row: the FFN down-projection finishes its row
 * (row_gemm_fr1_k launchable at this width); out[9] ... and the QKV projection runs in the same paired 8-channel form (2..8 finished rows: 2 = layers 1.. run it on rows_gemm_qp_k, 0 = on the 12-channel tiles); out[10] 2..8
 * finished rows: the FFN down-projection in the paired form (rows_gemm_frp_k); out[11] 17..64 rows: the layer runs on rows_gemm_wd_k
 * (1) or falls back to rows_gemm_mt_k (0); out[12] / out[13] its K slices for the out-projection / FFN down-projection; out[14] /
 * out[15] its k-tiles per wave for K = d / K = head_hidden.  tests/test_plan_cpu.py walks every model width with it. */
int vc_debug_plan(const vc_model_cfg* cfg, int compute_dtype, int rows, int32_t out[16]);
/* Host only: what option "w8r" = mask makes of a bf16 decode pass of `rows` rows at this model shape, every matrix taken as packed.
 * out[0] / out[1] = 1 when the FFN down-projection / the QKV projection of layers 1.. run on the E4M3 bytes (rows_gemm_frp_w8_k /
 * rows_gemm_qp_w8_k), out[2] / out[3] their groups per wave (0 where the form is not taken).  VC_EINVAL: a null pointer, rows < 1,
 * a mask with other bits than 1 and 4.  tests/test_w8_rows_cpu.py walks every model width with it. */
int vc_debug_w8r_plan(const vc_model_cfg* cfg, int mask, int rows, int32_t out[4]);
/* Host only: what option "w8m" = mask (bits 1 and 8) makes of a bf16 decode pass of `rows` rows at this model shape, the matrix taken
 * as packed.  out[0] = 1 when the FFN down-projection runs on the E4M3 bytes, out[1] the kernel (1 = rows_gemm_fr_w8_k, X in one piece;
 * 2 = rows_gemm_fr2_w8_k, K in two halves), out[2] its groups per wave and piece, out[3] = 0; all zeros where the form is not taken
 * (always up to 8 and from 17 rows).  VC_EINVAL: a null pointer, rows < 1, a mask with other bits.  tests/test_w8_mid_cpu.py walks
 * every model width. */
int vc_debug_w8m_plan(const vc_model_cfg* cfg, int mask, int rows, int32_t out[4]);
/* Host only: what option "w8w" = mask (bits 1, 4 and 8) makes of a bf16 decode pass of `rows` rows at this model shape, every matrix
 * taken as packed.  out[0] / out[1] = 1 when the FFN down-projection / the QKV projection run on the pair planes (rows_gemm_wds_w8_k),
 * out[2] / out[3] the k-tiles per wave of the FFN-down K slice / of the QKV matrix there (0 where the form is not taken).  All zeros
 * up to 16 rows.  VC_EINVAL: a null pointer, rows < 1, a mask with other bits.  tests/test_w8_wide_cpu.py walks every model width. */
int vc_debug_w8w_plan(const vc_model_cfg* cfg, int mask, int rows, int32_t out[4]);
/* Host only: what option "w8u" = mask (0, 2 or 10) makes of a bf16 decode pass of `rows` rows at this model shape, W1 taken as packed.
 * out[0] = 1 when the FFN up-projection runs on the pair planes (rows_gemm_wds_w8u_k), out[1] the k-tiles per wave there (0 where the
 * form is not taken).  Zeros up to 16 rows.  VC_EINVAL: a null pointer, rows outside 1..64, another mask.  tests/test_w8_up_cpu.py
 * walks every model width. */
int vc_debug_w8u_plan(const vc_model_cfg* cfg, int mask, int rows, int32_t out[2]);
/* Host only: what option "w8ur" = mask (0, 2 or 10) makes of a bf16 decode pass of `rows` rows at this model shape, W1 taken as packed.
 * out[0] = 1 when the FFN up-projection runs on the pair planes (rows_gemm_lnq_w8_k), out[1] the k-tiles per wave there (0 where the
 * form is not taken).  Zeros at 1 row and from 17 rows on.  VC_EINVAL: a null pointer, rows outside 1..64, another mask.
 * tests/test_w8_up_rows_cpu.py walks every model width. */
int vc_debug_w8ur_plan(const vc_model_cfg* cfg, int mask, int rows, int32_t out[2]);
/* Host only: what option "w8q" = mask (0, 4 or 12) makes of a bf16 decode pass of `rows` rows at this model shape, Wqkv taken as packed.
 * out[0] = 1 when the QKV projection of layers 1.. runs on the pairs of the 12-channel image (rows_gemm_qkvq_w8_k), out[1] the k-tiles
 * per wave there (0 where the form is not taken).  Zeros at 1 row, at the row counts the paired consumer takes and from 17 rows on.
 * VC_EINVAL: a null pointer, rows outside 1..64, another mask.  tests/test_w8_qkv_rows_cpu.py walks every model width. */
int vc_debug_w8q_plan(const vc_model_cfg* cfg, int mask, int rows, int32_t out[2]);
/* Host only: the packer of the "w8q" pairs (csrc/vc_w8.h, the text the device packer runs per lane) on n_pairs pairs of a 12-channel
 * bf16 image of KT k-tiles per tile (1536 B each: fragments of k-tiles 2j, 2j + 1 of one tile, 48 slots of 16 bytes, slot kg * 12 + m =
 * channel m, inputs 8 kg .. + 7 of its k-tile; pair P belongs to tile P / (KT / 2), whose parity places the split between the parts):
 * planes = n_pairs x 768 B, side = n_pairs x 2 bytes (shift + 127 of part 0, of part 1), *refused_pairs = pairs with a part off the
 * grid.  -1: a null pointer, n_pairs < 0 or no whole tiles, an odd KT. */
int vc_w8q_pack_host(const uint16_t* image12, long n_pairs, uint8_t* planes, uint8_t* side, int KT, int32_t* refused_pairs);
/* Host only: the packer of the pair planes (csrc/vc_w8.h, the text the device packer runs per lane) on n_pairs pairs of a 16-channel
 * bf16 image (2 KB each: fragments of k-tiles 2j, 2j + 1 of one tile, lane l = channel l & 15, inputs 8 (l >> 4) .. + 7 of its k-tile):
 * planes = n_pairs x 1 KB (16 bytes per lane: eight codes of k-tile 2j, eight of 2j + 1), side = n_pairs x 2 bytes (shift + 127 of
 * channels 0..7, of channels 8..15), *refused_pairs = pairs with a half off the grid.  Returns 0, or -1 on a null pointer. */
int vc_w8w_pack_host(const uint16_t* image16, long n_pairs, uint8_t* planes, uint8_t* side, int32_t* refused_pairs);
/* Copies a named internal device buffer to host memory.  "kcache<l>" / "vcache<l>": layer l's K / V cache, [max_seqs][H][max_positions][hd]
 * in the compute dtype; "eval_logits": see vc_eval_forward. */
int vc_debug_read(vc_engine* e, const char* name, void* host_dst, int64_t nbytes);
/* Timing of the last vc_tts/vc_edit call, measured with HIP events on `stream`:
 * ms[0] = prompt build + prefill, ms[1] = decode loop, ms[2] = their sum.  The FIRST call of a shape / option state captures and
 * instantiates its decode graphs before either timer starts (host time, in vc_debug_read "host_ms" [1] / [2]): neither figure holds it. */
int vc_last_timing(const vc_engine* e, float ms[3]);
/* Average duration in ms of ONE kernel of the decode step - `which` = "qkv" | "attn" | "oproj" | "ffn1" (the FFN up-projection: since
 * round 5 the longest launch of a one-row layer, the kernel bench.py's roofline object quotes) | "ffn2", "<name>_hot" (the same layer
 * every launch: cache-resident), "pf_ffn1" / "pf_qkv" / "pf_attn" (prefill block GEMM / tile attention, FLOPs instead of bytes),
 * "wd_qkv" | "wd_oproj" | "wd_ffn1" | "wd_ffn2" | "wd_ln" | "wd_attn" (the launches of a WIDE decode step, n_rows in 17..64) or "step"
 * (a whole decode step of up to 16 rows without the sampler) - in the form a step of `n_rows` rows really launches, measured with HIP
 * events over `iters` back-to-back launches on `stream` (layers rotate: cold caches), and the algorithmic bytes (FLOPs) one launch moves. */
int vc_bench_kernel(vc_engine* e, const char* which, int n_rows, int iters, float* avg_ms,
                    double* alg_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VC_ENGINE_H */
