// vc_engine_host.h - what the host units of libvcengine.so (vc_engine*.hip) share: the engine struct behind the C ABI of
// include/vc_engine.h, the plain structs that cross units, the decode loop's declaration and one prototype for every function
// called from another unit.  Private to csrc/; no torch types anywhere.
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <limits.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <deque>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "vc_common.h"

// Everything that crosses a unit lives in vch, hidden from the library's dynamic symbol table.  The attribute holds for the block it
// stands on, and a definition does not take it over from its declaration: the units reopen vch with the attribute too.  A helper
// of one unit stays in that unit's anonymous namespace.
namespace vch __attribute__((visibility("hidden"))) {

struct RawTensor {
  std::vector<int64_t> shape;
  float* dev = nullptr;   // fp32 staging copy in HBM
  long numel = 0;
};

struct Layer {
  uint4 *Wqkv = nullptr, *Wo = nullptr, *W1 = nullptr, *W2 = nullptr;
  uint4 *Wo8 = nullptr, *W28 = nullptr;                                 // Wo / W2 once more in 8-channel tiles (finished-row producers, vc_gemm.hip)
  uint4 *Wqkv16 = nullptr;                                              // Wqkv . gamma in 16-channel tiles (prefill and wide-decode passes, option "qkv16")
  uint4 *Wqkv8 = nullptr;                                               // Wqkv . gamma in 8-channel tiles (one-row paired QKV kernel, option "qkv_p8")
  float *bqkv = nullptr, *bo = nullptr, *b1 = nullptr, *b2 = nullptr;   // bqkv / b1 hold the FOLDED biases (W beta + b)
  float bo_mean = 0.f, b2_mean = 0.f;   // mean over the d channels of bo / b2: what the update moves a row's mean by whatever its input (GemmArgs.mu_shift)
  float *wg_qkv = nullptr, *wg_1 = nullptr;                             // row sums of the folded weights W . gamma
  void *kc = nullptr, *vc = nullptr;   // KV cache of this layer: WT [max_seqs][H][S_max][hd]
  // on request (vc_request_kv8): the same rows as E4M3 bytes, uint8 [max_seqs][H][S_max][hd], and their shifts, int8 [max_seqs][H][S_max][2] (K, V)
  unsigned char *kc8 = nullptr, *vc8 = nullptr;
  signed char* sh8 = nullptr;
  void* kcen = nullptr;      // on request (vc_request_kv8c): the K centres of this layer, bf16 [max_seqs][H][hd] (vc_kv8.h)
  // W28 / Wqkv8 once more in the packed forms of vc_packed (vc_common.h): [VC_PK_W13] exact 13-bit planes (option "w13", vc_w13.h) and, on request
  // (vc_request_w8), [VC_PK_W8] E4M3 bytes with one shift byte per fragment (option "w8", vc_w8.h); second index W13_F2 / W13_QKV.
  // A third slot, [PK_W8W], on request (vc_request_w8_wide): the 16-channel images W2 / Wqkv16 of wide steps as E4M3 PAIR planes
  // (option "w8w", vc_w8.h: 1 KB of codes + two side bytes per pair; `refused` counts pairs there).  That slot alone has a third
  // matrix, W13_F1, on request (vc_request_w8_up / vc_request_w8_up_rows): the pair planes of the FFN up-projection's image W1 (options "w8u", "w8ur")
  struct Packed {
    uint4* planes = nullptr;
    uint32_t* side = nullptr;      // one byte per fragment
    int state = 0;                 // 0 not applicable (or not packed), 1 packed, 2 refused: the launch stays on the bf16 image
    int refused = 0;               // fragments the packer refused
  } packed[VC_PK_N + 1][3];
  // on request (vc_request_w8_qkv_rows), layers 1..: the pairs of the 12-channel image Wqkv (option "w8q", vc_w8.h "w8q": 768 B of codes +
  // two side bytes per pair, one per part; `refused` counts pairs).  A slot of its own: [PK_W8W][W13_QKV] belongs to the 16-channel planes
  Packed w8q;
};
constexpr int PK_W8W = VC_PK_N;
enum { W13_F2 = 0, W13_QKV = 1, W13_F1 = 2 };
constexpr int W8_BITS[3] = {1, 4, 2};     // the mask bits of options "w13" / "w8" and of vc_request_w8 for W13_F2, W13_QKV; of "w8u" / "w8ur" and their requests for W13_F1

struct Plan { int n_tiles, KT, ksplit, nchunk; };

// Words of the pinned vc_engine::h_flag block.  HF_ACTIVE / HF_LIVE0..1 are written by the device (SampleArgs.host_active / host_live: the
// sequences still active; the two slots of "sequences still live as the LAST step of a batch found them"), HF_GATHER_N by stream_gather_k.
enum { HF_ERR = 0, HF_STAGE = 1, HF_SHARE = 2, HF_ACTIVE = 8, HF_LIVE0 = 9, HF_LIVE1 = 10, HF_LIVE_STEPS = 11, HF_GATHER_N = 12 };
// vc_engine::host_ms (vc_debug_read "host_ms": read by position): graph capture / instantiation of the last call, its decode loop's host
// time, the decode steps it LAUNCHED (a multiple of steps_per_graph; the tail are no-ops) and the re-packs that moved live sequences.
enum { HM_CAPTURE = 1, HM_INSTANTIATE = 2, HM_LOOP = 3, HM_SPARE = 4, HM_LAUNCHED = 5, HM_REPACKS = 6 };
// Session::stats (vc_session_stats: read by position; [7] is the admission time).  The row sums count every sample's rows.
enum { SS_ADMITTED = 0, SS_ADMITTED_LIVE = 1, SS_TURNS = 2, SS_WIDENINGS = 3, SS_NARROWINGS = 4, SS_LIVE_ROWS = 5, SS_LAUNCHED_ROWS = 6 };

}  // namespace vch
using namespace vch;   // struct vc_engine names these types unqualified, and so does every unit

struct vc_engine {
  vc_model_cfg cfg{};
  int device = 0;
  int dtype = -1;
  bool finalized = false;
  std::string err;
  std::map<std::string, RawTensor> raw;
  std::vector<void*> allocs;

  int d = 0, H = 0, hd = 0, L = 0, K = 0, V = 0, P = 0, S_max = 0, B_max = 0;
  int esz = 2;

  std::vector<Layer> layers;
  uint4 *Wh1 = nullptr, *Wh2 = nullptr;
  float *bh1 = nullptr, *bh2 = nullptr, *wg_h1 = nullptr;               // bh1: folded with the final LayerNorm
  long wh2_group_stride = 0;
  float *text_emb = nullptr, *audio_emb = nullptr, *mask_emb = nullptr, *pe = nullptr;
  float alpha_text = 1.f, alpha_audio = 1.f;
  Plan p_qkv{}, p_o{}, p_f1{}, p_f2{}, p_h1{}, p_h2{};
  Plan p_qkv16;                         // the same matrix on 16-channel tiles (Layer.Wqkv16)

  // activations / scratch
  float *emb = nullptr;                 // prefill rows [emb_cap][d] (one or several prompts back to back)
  int emb_cap = 0;
  int *pre_row_seq = nullptr, *pre_row_pos = nullptr;
  float *hA = nullptr, *hB = nullptr, *q = nullptr, *parts = nullptr, *att_o = nullptr, *att_ml = nullptr;
  void *act = nullptr, *hh = nullptr, *xn = nullptr;
  float *logits = nullptr;              // [B_max][K][V]
  float *dec_h = nullptr;               // [max(VC_ROWS, max_seqs)][d]
  int NS = VC_ROWS;                     // rows the per-sequence buffers are sized for
  int *dec_row_seq = nullptr, *dec_row_pos = nullptr, *logit_row = nullptr;
  SeqState *st = nullptr, *st_fin = nullptr;      // st_fin: final states by slot of sequences a re-pack moved out of the step (repack_k)
  long long* dbg_ts = nullptr;
  int *one = nullptr;                   // device word holding 1: the "always active" flag of prefill launches
  int *share_len = nullptr;             // device word: text positions shared with sequence 0 (AttnArgs.share_len), 0 outside such calls
  int *step_ctr = nullptr;              // SampleArgs.step_ctr
  int *n_active = nullptr, *samp = nullptr, *cond = nullptr, *amax = nullptr, *gen = nullptr, *err_flag = nullptr;
  int gen_cap = 0;
  // pinned host staging
  SeqState *h_st = nullptr, *h_st2 = nullptr;
  int *h_flag = nullptr;                // indexed by HF_*: error/poll word, staging, "sequences still active" written by the device,
                                        // SampleArgs.host_live, the decode loop's live steps (step_ctr, after a re-packed call)
  SampleDyn *h_dyn = nullptr, *d_dyn = nullptr;   // per-call sampler values (vc_common.h)
  // captured decode steps, kept across calls: key = (sequences, rows per sequence, best-of-N)
  // ... and by the option state they were captured under (vc_set_option): toggling an option back and forth reuses the captures
  std::map<std::pair<std::tuple<int, int, int>, std::string>, hipGraphExec_t> graphs;
  std::string opt_state;                // canonical text of every option that shapes a decode step
  int steps_per_graph = 8;              // VC_GRAPH_STEPS: decode steps captured into one graph launch
  hipEvent_t ev_pace[2]{};
  std::vector<int> repack_at;           // decode_loop: the batch index before which each re-pack of the last call was queued

  hipStream_t own_stream = nullptr;     // used when the caller passes the null stream (not capturable)
  hipStream_t side_stream = nullptr;    // vc_tts_stream_next gathers finished frames here: never behind the decode stream's queued graphs
  struct TtsStream* ts = nullptr;       // the open streaming TTS call (vc_tts_stream_begin .. vc_tts_stream_end), else NULL
  struct Session* sess = nullptr;       // the open decode session (vc_session_open .. vc_session_close), else NULL
  // decode sessions: per-slot Philox keys, the batch index the sampler stamps retirements with, where this turn's admitted rows start and
  // whose they are, prompt_k's error bits by slot, the prefill's own gather rows (the decode step's logit_row stays the live rows'), and the
  // pinned retirement records the host reads (vc_common.h VC_SESS_REC)
  uint64_t* seed_tab = nullptr;
  int* samp_tab = nullptr;  // [NS] by slot: sample index | sample count << 16 of the row's request (sessions opened for best-of-N requests)
  int *batch_id = nullptr, *row_base = nullptr, *adm_slot = nullptr, *prompt_err = nullptr, *sess_gather = nullptr;
  int* h_rec = nullptr;
  // ... the requests' sampling controls by slot (SampleDyn.ctl_tab), and the staging of a turn's admitted requests: their first states
  // and controls, written by the host into one of VC_ADM_STAGES pinned buffers (rotated by batch index, see vc_session_advance) and
  // uploaded on the decode stream into adm_st / adm_ctl in front of session_turn_k
  vc_request_ctl *ctl_tab = nullptr, *adm_ctl = nullptr, *h_adm_ctl = nullptr;
  SeqState *adm_st = nullptr, *h_adm_st = nullptr;
  // Non-temporal weight loads of the decode kernels, per matrix: bit 0 QKV, 1 out-projection, 2 FFN-up, 3 FFN-down, 4 heads-1, 5 heads-2.
  // Option "nt" (VC_NT).  Until round 4 the compiled QKV / out-projection / heads-2 kernels carried NO such load whatever this said (the
  // compiler merged the kernel's two load arms and dropped the hint): 28 reproduces that mix, 63 = every matrix (default), 0 = none.
  int nt_decode = 63;
  // option "nt", second value: the decode attention's K/V loads carry the hint too - 0 never, 1 always, 2 (default) from two rows per step up
  // (in-process A/Bs, profiles/r04d_bench_*attn_nt*: one row +0.3 % +- 0.09 - there the launch is latency-bound and carries the prefetch
  // role -, 8 rows -4.8 % +- 0.05, 32 rows -6.5 % +- 0.05: several caches stream 58-230 MB per layer through L2 otherwise)
  int attn_nt = 2;
  // finished-row form of passes of 2..fr_rows rows (plan_pass): 0 = off.  VC_FINISHED_ROWS / option "finished_rows"
  int fr_rows = VC_ROWS;
  // option "tile_attn": prefill attention kernel - 1 = tile_attn_k (16 query rows per wave, keys split over the waves), 2 =
  // tile_attn64_k (64 query rows per workgroup, transposed score product, P in registers; bf16 / head_dim 128 only, prompts are then
  // laid out on 64-row boundaries)
  // Default 2 when the call's longest prompt has at least 768 rows ("tile_attn" = "k[,min_rows]"): measured on one layer of giga830M (profiles/r04o_attn64_probe.log)
  // 512 / 800 / 2048 causal rows: 14.3 / 24.6 / 86.7 us (first kernel) against 15.5 / 21.0 / 52.5 us (second).
  int tile_attn = 2, tile_attn_min_rows = 768;
  // option "fr_one" (round 5): ONE-row steps - the FFN down-projection finishes its row (row_gemm_fr1_k: 8-channel tiles over the whole K,
  // two k-tiles per MFMA fragment, residual + bias added) instead of leaving 4 split-K slabs, so the next layer's QKV projection (and
  // heads-1) reads one 8 KB row instead of h + bias + 4 slabs = 40 KB in each of its 512 workgroups; 0 = off
  int fr_one = 1;
  // option "fr_pair" (round 5): the FFN down-projection of 2..8-row steps with two k-tiles per MFMA fragment (rows_gemm_frp_k) instead
  // of half-filled 8-channel fragments (rows_gemm_fr_k)
  int fr_pair = 1;
  // option "qkv_p8" (round 5): one-row steps behind a finished row (fr_one) run the QKV projection on 8-channel tiles with two k-tiles
  // per MFMA fragment (row_gemm_fr1_k<PRO_LN, EPI_QKV>: every lane's 16 bytes are weights) instead of 12-channel tiles; 2 (round 6): steps of
  // 2..8 finished rows too, behind the producers' centred copy (rows_gemm_qp_k)
  int qkv_p8 = 2;
  // option "qkv16" (round 5): prefill passes and wide decode passes (17..64 rows) run the QKV projection on a 16-channel image of the
  // folded matrix (every A lane of every MFMA a weight) instead of the 12-channel tiles one-row steps were tuned on; + 6 d^2 bytes per
  // layer in bf16 (0.4 GB at giga830M).  Packed for engines that can take wide steps (max_seqs > 16) or with VC_QKV16=1 at creation;
  // otherwise the option stays off and prefill passes read the 12-channel tiles.
  int qkv16 = 1;
  // option "wide_heads" (round 5): decode steps of 17..64 rows run the prediction heads once on the weight-stationary kernel of those
  // steps (one LayerNorm launch + two rows_gemm_mt_k launches) instead of once per 16 rows on the rows-GEMM
  int wide_heads = 1;
  // option "wide_gemm" (round 6): the linear layers of 17..64-row steps on rows_gemm_wd_k (vc_gemm_wd.hip: every row tile of the step in
  // flight at once, X fragments straight from L2 into registers, one barrier per launch) instead of the weight-stationary
  // rows_gemm_mt_k, which walks the row tiles one after the other; 0 = that kernel (two weight tiles per workgroup)
  int wide_gemm = 1;
  // option "wd_stage": 1 (default) = that kernel takes X as whole cache lines through a wave-private LDS stage (rows_gemm_wds_k: 64 rows FFN-up
  // 13.5 -> 9.7 us, the 64-row step -9.5 % +- 0.01, 32 rows -2.7 %; profiles/r06c_*), 0 = MFMA fragments straight from L2 (16 half lines per request)
  int wd_stage = 1;
  // option "shrink" (round 6): a multi-utterance call whose sequences retire at different steps re-packs the live ones onto the rows of a
  // narrower step (the next power of two >= the live count: 64 -> 32 -> 16 -> 8 -> 4 -> 2 -> 1) instead of keeping its launch form until
  // the longest sequence ends; 0 = the fixed width of rounds 1-5.  Results do not depend on it: everything per sequence is indexed by its slot.
  int shrink = 1;
  // weight images vc_finalize_weights packed: Layer.Wo8 / W28, Layer.Wqkv8, Layer.Wqkv16 (the forms that read one, plan_pass)
  bool has_fr8 = false, has_qkv8 = false, has_qkv16 = false;
  // option "w13": one-row steps stream the FFN down-projection (1) and the QKV projection (4) as exact 13-bit planes of the same bf16
  // values (vc_gemm_w13.hip: 13/16 of the bytes, results bit-identical).  bf16 engines; planes packed at creation unless VC_W13=0
  // (+ 0.81 x the two images: 0.76 GB at giga830M); a matrix the packer refuses keeps its bf16 launch.  (Bit 2, the FFN up-projection, was
  // built and measured +0.1 % +- 0.03 per step: it left the tree with its kernel)
  int w13 = 5;
  bool has_w13 = false;
  unsigned int* w13_counts = nullptr;   // two device words of the packer: fragments refused, dwords that did not decode to the image
  // option "w8": the same two launches stream E4M3 bytes + one shift byte per fragment (vc_gemm_w8.hip: half the bytes of the image,
  // results bit-identical) for matrices that lie on that grid (voicecraft_amd/quant.py).  Only on an engine that asked for it before
  // vc_finalize_weights (vc_request_w8: w8_req); a matrix off the grid is refused and keeps its current launch.  Where a matrix has both
  // kinds of planes the w8 bit wins.  An engine without the request packs nothing and has no such option.
  int w8_req = 0;
  int w8 = 0;
  // option "w8r": steps of 2..8 finished rows stream the same planes - the FFN down-projection (1) on rows_gemm_frp_w8_k, the QKV
  // projection of layers 1.. (4) on rows_gemm_qp_w8_k, results bit-identical -, where plan_pass takes the form.  Only on an engine
  // that asked for it after vc_request_w8 (vc_request_w8_rows: w8r_req, a subset of w8_req); any other engine has no such option
  // and launches what it launched before.
  int w8r_req = 0;
  int w8r = 0;
  // option "w8m": passes of 9..16 finished rows stream the FFN down-projection (1) from the same planes (rows_gemm_fr_w8_k /
  // rows_gemm_fr2_w8_k: the image kernels' text, one decoded fragment feeding two k-tiles, results bit-identical), where plan_pass
  // takes the form; bit 8 = also at row counts the win table (w8_rows_win, W8_FORMS below) leaves out, for the A/B tool and the tests.  Only on an
  // engine that asked for it after vc_request_w8 (vc_request_w8_mid: w8m_req, a subset of w8_req; QKV has no consumer of Wqkv8 at
  // these row counts).  Nothing more is packed; any other engine has no such option and launches what it launched before.
  int w8m_req = 0;
  int w8m = 0;
  // option "w8w": steps of 17..64 rows stream the FFN down-projection (1) and the QKV projection (4) as E4M3 pair planes of their
  // 16-channel images W2 / Wqkv16 (rows_gemm_wds_w8_k: the staged wide kernel's text on half the weight bytes, results bit-identical),
  // where plan_pass takes the form; bit 8 = also at row counts the win table (w8_rows_win, W8_FORMS below) leaves out, for the A/B tool and the
  // tests.  Only on an engine that asked for it after vc_request_w8 (vc_request_w8_wide: w8w_req, a subset of w8_req) and that can
  // run wide steps (has_qkv16): + 0.5 x the two images resident (7 d^2 bytes per layer: + 0.47 GB at giga830M).  Any other engine
  // packs nothing more, has no such option and launches what it launched before.
  int w8w_req = 0;
  int w8w = 0;
  // option "w8u": steps of 17..64 rows stream the FFN up-projection (2) as E4M3 pair planes of its 16-channel image W1
  // (rows_gemm_wds_w8u_k: the same text with the bias + ReLU epilogue, results bit-identical), where plan_pass takes the form; bit 8 =
  // also at row counts the win table (w8_rows_win, W8_FORMS below) leaves out, for the A/B tool and the tests.  Only on an engine that asked for it
  // after vc_request_w8 (vc_request_w8_up: w8u_req = 2) and that can run wide steps (has_qkv16): + 0.5 x the W1 image resident
  // (4 d^2 + d^2 / 128 bytes per layer: + 0.27 GB at giga830M).  Independent of "w8w".  Any other engine packs nothing more, has
  // no such option and launches what it launched before.
  int w8u_req = 0;
  int w8u = 0;
  // option "w8ur": passes of 2..16 finished rows stream the FFN up-projection (2) from the SAME pair planes of W1 (rows_gemm_lnq_w8_k: the
  // text of rows_gemm_k<bf16_t, KTW, PRO_LNQ, EPI_RELU, ..> with the pairs as the weight source, results bit-identical), where plan_pass
  // takes the form; bit 8 = also at row counts the win table (w8_rows_win, W8_FORMS below) leaves out, for the A/B tool and the tests.  Only on an
  // engine that asked for it after vc_request_w8 (vc_request_w8_up_rows: w8ur_req = 2), whatever its max_seqs: + 0.5 x the W1 image
  // resident (4 d^2 + d^2 / 128 bytes per layer: + 0.27 GB at giga830M) unless "w8u" holds the planes already.  Any other engine packs
  // nothing more, has no such option and launches what it launched before.
  int w8ur_req = 0;
  int w8ur = 0;
  // option "w8q": passes of finished rows whose QKV projection still launches rows_gemm_k<bf16_t, KTW, PRO_LNQ, EPI_QKV, ..> on the
  // 12-channel image (the row counts past the paired consumer's, p.qp: 9..16 everywhere, 7 and 8 at d = 2048; with qkv_p8 < 2 also the
  // lower ones) stream the QKV projection (4) of layers 1.. from the pairs of that image (rows_gemm_qkvq_w8_k: the same text with the
  // pairs as the weight source, results bit-identical), where plan_pass takes the form; bit 8 = also at row counts the win table
  // (w8_rows_win, W8_FORMS below) leaves out, for the A/B tool and the tests.  Only on an engine that asked for it after vc_request_w8
  // (vc_request_w8_qkv_rows: w8q_req = 4), whatever its max_seqs: + 0.5 x the Wqkv image resident per packed layer (3 d^2 + d^2 / 128
  // bytes: + 0.20 GB at giga830M).  Any other engine packs nothing more, has no such option and launches what it launched before.
  int w8q_req = 0;
  int w8q = 0;
  // option "kv8": decode passes read the cached positions older than the pass from an E4M3 copy of the K / V cache (Layer.kc8 / vc8 / sh8,
  // vc_kv8.h: one byte per value, one shift per cached row of a head - half the bytes of the launch that grows with the batch), which
  // one kv8_pack_k launch behind every pass keeps equal to the quantiser of the bf16 rows.  This changes values (3 mantissa bits), so:
  // only on an engine that asked for it before vc_finalize_weights (vc_request_kv8: kv8_req); 0 = such an engine reads bf16 again (it
  // goes on packing).  An engine without the request allocates nothing, launches nothing more and has no such option.
  int kv8_req = 0;
  int kv8 = 0;
  Kv8Layer* kv8_tab = nullptr;          // device table [L] of the layers' five arrays (Kv8PackArgs.layers)
  // "kv8c" (vc_request_kv8c, implies the above; the contract is in vc_kv8.h): K meets the grid as k - c, c the mean K row of the prefill
  // pass that wrote the slot's position 0, per layer, slot and head (Layer.kcen; kv8c_centre_k in front of the packer on prefill passes);
  // the decode attention adds q . c to its 8-bit scores.  Fixed at creation: option "kv8" switches between this and the bf16 cache.
  int kv8c_req = 0;
  void** kcen_tab = nullptr;            // device table [L] of the layers' centre arrays
  int* kcen_rows = nullptr;             // device [max_seqs]: n0, the rows each slot's centre is the mean of
  int cur_rows = 0;                     // rows per step the last decode loop ended on (tts_run reads the states back accordingly)
  // option "attn_fast": decode attention with the wave's maximum taken before any exponential (no online rescaling inside a wave) and,
  // in bf16 mode, hardware exp2 (v_exp_f32) instead of expf
  int attn_fast = 1;
  // option "hq" (round 6): the finished-row producers of 2..16-row steps also write their rows CENTRED and in the compute dtype (hqA / hqB =
  // WT(h - c), c = the row's mean as the previous LayerNorm found it: row_mu ping-pong), and the LayerNorm-folding consumers read that copy
  // (PRO_LNQ: half the bytes of the fp32 row in bf16 mode, no conversion) - the fold is exact for any centring constant
  int hq = 1;
  void *hqA = nullptr, *hqB = nullptr;  // centred copies of hA / hB, WT [VC_ROWS][d]
  float* row_mu[2] = {nullptr, nullptr};       // [VC_ROWS] each: ping-pong of the rows' means
  float* mu_zero = nullptr;             // [VC_ROWS] zeros: GemmArgs.row_mu of every launch that centres nothing
  // option "att_p16" (round 6; bf16 mode): finished-row passes of 2..8 rows hand the attention's split partials to the out-projection as
  // bf16 (131 -> 66 KB per out-projection workgroup at 8 rows; the merged row is rounded to bf16 for the MFMA anyway)
  int att_p16 = 1;
  static constexpr int attn_blocks_multi = 512, attn_blocks_one = 256;   // attention workgroups aimed at (several rows / one row); 256 -> 64 at one row measured +1.1..+1.8 % (r05f)
  int prefill_rows_per_pass = VC_MAX_ROWS;   // VC_PREFILL_ROWS=16 falls back to the decode kernels for the prompt
  hipEvent_t ev[3]{};
  float ms[3]{0, 0, 0};
  double host_ms[8]{};                  // host wall clock of the last call's phases, indexed by HM_* (vc_debug_read "host_ms")
  double bytes_total = 0;               // HBM bytes owned by the engine
  // training objective (vc_eval_forward), allocated on first use
  int *ce_tgt = nullptr, *ce_hit = nullptr;
  float *ce_nll = nullptr;
  double *ce_sum = nullptr;
  long long *ce_hits = nullptr, *ce_cnt = nullptr;
  // parity hook of vc_eval_forward (nll_dev / tgt_dev given): the head logits of every row of the last such call, [rows][K][V]
  // (vc_debug_read "eval_logits"); allocated by the first call that asks for it and grown on demand, never otherwise
  float *eval_logits = nullptr;
  int64_t eval_logits_cap = 0, eval_logits_rows = 0;      // rows allocated / rows the last call left
};

#define VC_ADM_STAGES 4
static_assert(sizeof(vc_request_ctl) == 16, "vc_request_ctl is copied as one 16-byte quad (vc_tokens.hip session_turn_k)");

namespace vch __attribute__((visibility("hidden"))) {

inline double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int fail(vc_engine* e, int code, const char* fmt, ...);      // vc_engine.hip

#define HIPCHK(e, call)                                                                  \
  do {                                                                                   \
    hipError_t _err = (call);                                                            \
    if (_err != hipSuccess)                                                              \
      return fail(e, VC_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_err), \
                  __FILE__, __LINE__);                                                   \
  } while (0)

template <typename T>
int dalloc(vc_engine* e, T** p, size_t n) {
  void* v = nullptr;
  hipError_t err = hipMalloc(&v, std::max<size_t>(n * sizeof(T), 16));
  if (err != hipSuccess) return fail(e, VC_EHIP, "hipMalloc(%zu bytes) failed: %s", n * sizeof(T), hipGetErrorString(err));
  e->allocs.push_back(v);
  e->bytes_total += (double)(n * sizeof(T));
  *p = reinterpret_cast<T*>(v);
  return VC_OK;
}
// the void* fields (buffers in the compute dtype): sized in bytes
inline int dalloc(vc_engine* e, void** p, size_t bytes) {
  char* c = nullptr;
  const int rc = dalloc(e, &c, bytes);
  *p = c;
  return rc;
}

// ---------------------------------------------------------------- the plain structs that cross units
struct RowSrc {
  const float* h_in;
  const int* row_seq;
  const int* row_pos;
  int n_rows;       // rows carried
  const int* n_active;
  int nt;           // force the streaming-load policy (microbenchmarks)
  int rps;          // decode passes: rows per sequence (1 or 3: consecutive rows at consecutive positions); 0: a prefill pass (option "kv8")
};

// Every launch decision of a pass of `rows` rows: plan_pass below is the one place they are made.
struct PassPlan {
  int form;         // FORM_*
  int attn;         // ATT_*
  int nsplit;       // attention splits
  bool att_x;       // the attention is unsplit and normalises its rows into xn; the out-projection takes them with the plain prologue
  bool part16;      // the split partials in bf16 (option att_p16)
  bool ln_launch;   // QKV / FFN-up: LayerNorm as its own per-row launch (ln_rows_k) + the plain prologue, else in the GEMM prologue
  bool hq;          // finished rows: the consumers fold the producers' centred copy (PRO_LNQ) instead of the fp32 rows (PRO_LNW)
  int mt;           // GemmArgs.mt of the consumers: 0 / 3 / 4 finished rows, 2 wide, 1 block
  bool fd;          // one row: the FFN down-projection finishes its row (row_gemm_fr1_k, option fr_one)
  bool qkv_fr1;     // ... and the QKV projection behind it pairs k-tiles on the 8-channel image (option qkv_p8)
  bool qp;          // 2..8 finished rows: the QKV projection of layers 1.. on rows_gemm_qp_k (qkv_p8 = 2)
  bool frp;         // finished rows: the FFN down-projection on rows_gemm_frp_k (option fr_pair)
  bool frp_w8;      // ... on the E4M3 bytes of a layer whose W28 is packed that way (rows_gemm_frp_w8_k, option w8r bit 1)
  bool qp_w8;       // qp on the E4M3 bytes of a layer whose Wqkv8 is packed that way (rows_gemm_qp_w8_k, option w8r bit 4)
  bool fr_w8_f2;    // 9..16 finished rows: the FFN down-projection on the E4M3 bytes of a layer whose W28 is packed that way (rows_gemm_fr_w8_k / rows_gemm_fr2_w8_k, option w8m bit 1)
  bool qkv16;       // wide and block: the QKV projection on the 16-channel image (option qkv16)
  bool wd;          // wide: the linear layers on rows_gemm_wd_k (option wide_gemm)
  bool wd_w8_f2;    // ... the FFN down-projection on the pair planes of a layer whose W2 is packed that way (rows_gemm_wds_w8_k, option w8w bit 1)
  bool wd_w8_qkv;   // ... the QKV projection on the pair planes of a layer whose Wqkv16 is packed that way (option w8w bit 4)
  bool lnq_w8_f1;   // finished rows behind a centred copy: the FFN up-projection on the pair planes of a layer whose W1 is packed that way (rows_gemm_lnq_w8_k, option w8ur bit 2)
  bool qkvq_w8;     // finished rows behind a centred copy, past the paired consumer's row counts: the QKV projection on the pairs of the 12-channel image of a layer whose Wqkv is packed that way (rows_gemm_qkvq_w8_k, option w8q bit 4)
  bool wd_w8_f1;    // ... the FFN up-projection on the pair planes of a layer whose W1 is packed that way (rows_gemm_wds_w8u_k, option w8u bit 2)
  int ks_o, ks_f2;  // split-K slabs the out-projection / FFN down-projection leave (slab, wide and block forms)
  bool heads_wide;  // the heads run once over all rows on the wide-step kernels (option wide_heads)
  bool heads_fold;  // heads-1 folds the finished rows itself (no LayerNorm launch)
};

// ---------------------------------------------------------------- the w8 forms, one row per option
// Everything vc_engine.hip knows about an option that streams E4M3 weights, apart from the launch itself: its request (request_w8_form),
// the values it accepts (w8_value_ok: the option table and the vc_debug_w8*_plan entry points), and the row counts at which plan_pass
// takes the form without being told to (w8_rows_win).  struct vc_engine says what each option does; DESIGN.md has the table in prose.
struct W8Form {
  const char *option, *request;             // the option's name, the C function that asks for it before vc_finalize_weights
  int vc_engine::*req, vc_engine::*value;   // what the request stored (0: no such option on this engine), the option's value
  int bits;                                 // the matrices of the form: 1 FFN-down, 4 QKV, 2 FFN-up
  // subset: the request takes any mask of vc_request_w8's bits 1 and 4 that is a subset of that request's (0 included; a bit outside
  // `bits` is refused behind that with `no_form`), the option any mask of `bits`.  Otherwise the request needs vc_request_w8 but none of
  // its bits and takes `bits` alone; the option takes 0 or `bits`.
  bool subset;
  bool every_rows;                          // the option's value has bit 8: also at the row counts rows_lo..rows_hi leaves out (the A/B tools, the tests)
  int rows_lo, rows_hi;                     // the row counts the measured table takes
  const char *mask_text, *value_text, *no_form;      // for the refusals: the request's masks, the option's values, a bit without a form
};
enum { W8F_ONE = 0, W8F_ROWS, W8F_MID, W8F_WIDE, W8F_UP, W8F_UP_ROWS, W8F_QKV_ROWS, W8F_N };
inline const W8Form W8_FORMS[W8F_N] = {
    // "w8": one-row steps; the request that packs the planes the next three read
    {"w8", "vc_request_w8", &vc_engine::w8_req, &vc_engine::w8, 5, true, false, 1, 1,
     "a mask of 1 (FFN-down) and 4 (QKV)", "a mask of 1 (FFN-down) and 4 (QKV)", nullptr},
    // "w8r": the row counts at which the w8 form of a matrix measured faster than the image over the whole paired range; a row count
    // whose range touches zero would stay on the image.  profiles/w8_rows_ab.log (giga830M, 7 interleaved pairs per line, captured
    // decode loop per step, min..max of the pairs): FFN-down alone -6.3 .. -5.8 % at 2, 3, 4, 6 and 8 rows, QKV alone -4.4 .. -5.0 % at
    // 2, 3, 4 and 6 rows (rows_gemm_qp_k stops at 6 rows at d = 2048), both -10.8 .. -11.0 %: every row count of both bits takes the form.
    {"w8r", "vc_request_w8_rows", &vc_engine::w8r_req, &vc_engine::w8r, 5, true, false, 2, 8,
     "a mask of 1 (FFN-down) and 4 (QKV)", "a mask of 1 (FFN-down) and 4 (QKV)", nullptr},
    // "w8m": the row counts of 9..16 at which the w8 form of the FFN down-projection measured faster than the image over the whole
    // paired range; a count that was not measured follows the nearest measured one.  profiles/w8_mid_ab.log (tools/w8_mid_ab.py:
    // giga830M, 7 interleaved pairs per line, captured decode loop per step, min..max of the pairs) at 9, 12, 16 rows: -5.3 .. -5.2 %,
    // -5.0 .. -4.9 %, -5.2 .. -5.2 %, and -4.8 .. -4.7 % for 16 utterances at the benchmark's shapes with `w8r` and `w8w` on: every measured
    // row count has its whole range below zero, so every row count 9..16 takes the form.
    {"w8m", "vc_request_w8_mid", &vc_engine::w8m_req, &vc_engine::w8m, 1, true, true, VC_FR_MAX_ROWS + 1, VC_ROWS,
     "a mask of 1 (FFN-down)", "a mask of 1 (FFN-down) and 8 (every row count)",
     "bit 4 (QKV) has no form - no kernel reads Wqkv8 at 9..16 rows; the mask is 1 (FFN-down)"},
    // "w8w": the row counts at which the pair-plane form of a matrix measured faster than the image over the whole paired range; row
    // counts between measured ones follow the nearest measured count of the same RT (17..32, 33..64).  profiles/w8_wide_ab.log
    // (tools/w8_wide_ab.py: giga830M, 7 interleaved pairs per line, captured decode loop per step, min..max of the pairs) at 17, 24,
    // 32 | 33, 48, 64 rows: FFN-down alone -4.9 .. -3.5 % | -3.6 .. -2.9 %, QKV alone -3.1 .. -2.9 % | -2.3 .. -2.0 %, both -7.9 .. -7.3 % |
    // -5.6 .. -5.2 %: every measured row count of both bits has its whole range below zero, so every wide row count takes the form.
    {"w8w", "vc_request_w8_wide", &vc_engine::w8w_req, &vc_engine::w8w, 5, true, true, VC_ROWS + 1, VC_MAX_SEQS,
     "a mask of 1 (FFN-down) and 4 (QKV)", "a mask of 1 (FFN-down), 4 (QKV) and 8 (every row count)", nullptr},
    // "w8u": the row counts at which the pair-plane form of the FFN up-projection measured faster than the image over the whole paired
    // range; row counts between measured ones follow the nearest measured count of the same RT (17..32, 33..64).  profiles/w8_up_ab.log
    // (tools/w8_up_ab.py: giga830M, 7 interleaved pairs per line, captured decode loop per step, min..max of the pairs) at 17, 24, 32 |
    // 33, 48, 64 rows: FFN-up alone -4.4 .. -4.0 % | -3.1 .. -2.6 %, next to `w8w` = 13 -4.9 .. -4.2 % | -3.3 .. -2.9 %, with kv8
    // -4.2 .. -4.1 % at 32 rows and -2.9 .. -2.8 % at 64: every measured row count has its whole range below zero, so every wide row
    // count takes the form.
    {"w8u", "vc_request_w8_up", &vc_engine::w8u_req, &vc_engine::w8u, 2, false, true, VC_ROWS + 1, VC_MAX_SEQS,
     "the mask 2 (FFN-up)", "0, 2 (FFN-up) or 10 (at every row count)", nullptr},
    // "w8ur": the row counts of 2..16 at which the pair-plane form of the FFN up-projection measured faster than the image over the
    // whole paired range; a count that was not measured follows the nearest measured one of the same kernel form (2..4, 5..8, 9..16
    // rows).  profiles/w8_up_rows_ab.log (tools/w8_up_rows_ab.py: giga830M, 7 interleaved pairs per line, captured decode loop per
    // step, min..max of the pairs) at 2, 4 | 5, 8 | 9, 12, 16 rows: -7.9 .. -7.5 % | -5.6 .. -4.9 % | -4.2 .. -3.7 %, and -5.3 % / -3.7 % for
    // 8 / 16 utterances at the benchmark's shapes with `w8r` and `w8m` on: every measured row count has its whole range below zero, so
    // every row count 2..16 takes the form.
    {"w8ur", "vc_request_w8_up_rows", &vc_engine::w8ur_req, &vc_engine::w8ur, 2, false, true, 2, VC_ROWS,
     "the mask 2 (FFN-up)", "0, 2 (FFN-up) or 10 (at every row count)", nullptr},
    // "w8q": the row counts at which the pair form of the QKV projection's 12-channel image measured faster than the image over the
    // whole paired range; a count that was not measured follows the nearest measured one of the same kernel form (2..4, 5..8, 9..16
    // rows).  profiles/w8_qkv_rows_ab.log (tools/w8_qkv_rows_ab.py: giga830M, 7 interleaved pairs per line, captured decode loop per
    // step, min..max of the pairs) at 7, 8 | 9, 12, 16 rows: -2.8 .. -2.6 % | -1.8 .. -1.5 %, and -1.6 .. -1.5 % for 16 utterances at the
    // benchmark's shapes with `w8r`, `w8m` and `w8ur` on: every measured row count has its whole range below zero, so 5..8 rows (two
    // tiles per workgroup) and 9..16 rows (two rows per wave as well) take the form where the 12-channel image serves them.  No count
    // of the one-tile form (2..4 rows, which the image serves with `qkv_p8` below 2 only) was measured: those stay out and reach the
    // kernel through bit 8.
    {"w8q", "vc_request_w8_qkv_rows", &vc_engine::w8q_req, &vc_engine::w8q, 4, false, true, 5, VC_ROWS,
     "the mask 4 (QKV)", "0, 4 (QKV) or 12 (at every row count)", nullptr},
};
inline bool w8_rows_win(int form, int rows) { return rows >= W8_FORMS[form].rows_lo && rows <= W8_FORMS[form].rows_hi; }
inline bool w8_value_ok(const W8Form& f, int v) {
  const int every = f.every_rows ? 8 : 0;
  return f.subset ? v >= 0 && !(v & ~(f.bits | every)) : v == 0 || v == f.bits || v == (f.bits | every);
}

// What a pass leaves for the heads in hB: finished rows (n_parts = 0; hq: their centred copy, on the means in mu) or rows whose
// n_parts split-K slabs and last FFN-down bias are still to be added.
struct PassOut { int n_parts; const void* hq; const float* mu; };

struct TtsJob { const int64_t* x; int Lx; const int64_t* y; int T; };

// One editing request: its inputs, the prefill's segment table (PromptArgs) and its budget of sampled steps.
struct EditJob {
  const int64_t* x; int Lx; const int64_t* y; int T;
  const int32_t* iv; int M; const int32_t* mv;     // mask intervals [M][2], mask values [2M]
  std::vector<int> ns, ne;                          // the M + 1 non-masked pieces
  PromptArgs pa;
  int max_steps;
};

// The loop as a resumable object: begin / advance / finish.  The blocking calls drive it to its end in one go (decode_loop); the
// streaming TTS call (vc_tts_stream_*) keeps it in the engine and advances it from vc_tts_stream_next, reading in between how many
// steps the pacing has shown to be complete.  One copy of the pacing and of the graph cache.
// groups: 0 = independent sequences, else the number of best-of-N groups the B0 sequences form (grouped sampler launches).
struct DecodeLoop {
  vc_engine* e = nullptr;
  SampleArgs sa{};
  vc_sample_cfg sc{};
  int B0 = 0, B = 0, rps = 1, groups = 0, G = 1, max_steps = 0;
  bool grouped = false, can_shrink = false;
  bool sess = false;       // the steps of a decode session (sample_session_k): graphs of their own
  hipStream_t s = nullptr;
  int launched = 0, batch = 0;
  int complete = 0;        // decode steps the host KNOWS to have ended (the pacing event behind them was waited for)
  bool over = false;       // nothing more will be queued: the last sequence retired, or the step budget is used up
  double t1 = 0;

  void init(vc_engine* e_, const SampleArgs& sa0, int B0_, int rps_, int groups_, const vc_sample_cfg* sc_, int max_steps_, hipStream_t s_);
  static int width_for(int live);
  int exec_for(hipGraphExec_t* out);
  int precapture();
  int begin();
  int queue_batch(int slot);
  int advance();
  void finish(int* steps_run);
};

// ---------------------------------------------------------------- vc_engine.hip
int check_idle(vc_engine* e);
int check_err_flag(vc_engine* e, hipStream_t s);
PassPlan plan_pass(const vc_engine* e, int rows, bool decode, int tiled);
int run_pass(vc_engine* e, const PassPlan& p, const RowSrc& rs, PassOut* out, hipStream_t s);
int run_heads(vc_engine* e, const PassPlan& p, const PassOut& po, const int* gather, int n, int in_row0, int out_row0,
              const int* n_active, hipStream_t s);
int prefill_batch(vc_engine* e, std::vector<PromptArgs>& pas, const std::vector<int>& slots, hipStream_t s, bool sess = false);
void fill_prompt_common(vc_engine* e, PromptArgs& pa, const int64_t* x, int Lx, const int64_t* y, int T);
SampleArgs make_sample_args(vc_engine* e, int B, int rps);
int push_sample_dyn(vc_engine* e, const vc_sample_cfg* sc, const int64_t* forced, int n_forced, float* logits_out,
                    int logit_steps, int n_seq, hipStream_t s, int n_group = 1);
SeqState tts_request(vc_engine* e, const TtsJob& j, int skip, const int64_t* x_shared, PromptArgs* pa);
int replicate_kv(vc_engine* e, CopyKvArgs kv, hipStream_t s);
int assemble_tts(vc_engine* e, const TtsJob& j, int slot, const SeqState& st, int64_t* res, int res_cap, int* gen_len, hipStream_t s);
int edit_prepare(vc_engine* e, EditJob& j, const char* who);
SeqState edit_state(vc_engine* e, const EditJob& j);
int edit_assemble(vc_engine* e, const EditJob& j, const SeqState& fs, const int* gen, int64_t* res, int res_cap, int* res_len,
                  hipStream_t s, const char* who);

// ---------------------------------------------------------------- vc_engine_session.hip
void drop_session(vc_engine* e);
int debug_session_slots(vc_engine* e, std::vector<int32_t>& out);      // vc_debug_read "session_slots"

}  // namespace vch
