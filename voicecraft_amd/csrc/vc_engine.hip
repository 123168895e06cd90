// vc_engine.hip — host side of libvcengine.so: the C ABI of include/vc_engine.h, HBM arena
// management, weight packing, prefill scheduling, the decode loop (eager or hipGraph replay) and
// output assembly.  No torch types anywhere; the caller hands raw device pointers and a stream.
//
// Control flow restated from VoiceCraft.inference_tts / inference_tts_batch / inference
// (models/voicecraft.py:908-1153, :1156-1439, :561-906); see DESIGN.md §2 for the mapping.
#include "vc_engine_host.h"
#include "vc_w8.h"      // the pair planes' sizes (pack_pairs)

namespace {

std::string g_create_err;

}  // namespace
namespace vch __attribute__((visibility("hidden"))) {
int fail(vc_engine* e, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (e) e->err = buf; else g_create_err = buf;
  return code;
}
}  // namespace vch
namespace {

Plan make_plan(int N, int Kdim, int dtype, bool allow_split, const char* env_override, int th = 16) {
  Plan p;
  const int KW = dtype == VC_DTYPE_BF16 ? 32 : 16;
  p.n_tiles = (N + th - 1) / th;
  p.KT = Kdim / KW;
  p.ksplit = 1;
  if (allow_split) {
    // grow the grid towards ~2 blocks per CU while every wave still streams >= 8 KiB per chunk
    while (p.n_tiles * p.ksplit < 512 && p.ksplit < VC_MAX_KSPLIT && (p.KT / (p.ksplit * 2)) >= 32 &&
           (p.KT % (p.ksplit * 2 * 8)) == 0)
      p.ksplit *= 2;
    if (env_override) {
      const char* v = getenv(env_override);
      if (v) {
        const int ks = atoi(v);
        if (ks >= 1 && ks <= VC_MAX_KSPLIT && p.KT % (ks * 8) == 0) p.ksplit = ks;
      }
    }
  }
  const int per = p.KT / p.ksplit;
  int ktw = 16;
  while (ktw > 2 && per % (4 * ktw) != 0) ktw >>= 1;
  p.nchunk = per / (4 * ktw);
  return p;
}

const RawTensor* find_raw(vc_engine* e, const std::string& key) {
  auto it = e->raw.find(key);
  return it == e->raw.end() ? nullptr : &it->second;
}

int need(vc_engine* e, const std::string& key, std::initializer_list<int64_t> shape, const RawTensor** out) {
  const RawTensor* t = find_raw(e, key);
  if (!t) return fail(e, VC_EMISSING, "weight '%s' was never loaded", key.c_str());
  std::vector<int64_t> want(shape);
  if (t->shape != want) {
    std::string got, exp;
    for (auto v : t->shape) got += std::to_string(v) + ",";
    for (auto v : want) exp += std::to_string(v) + ",";
    return fail(e, VC_EINVAL, "weight '%s' has shape [%s] but the config implies [%s]", key.c_str(), got.c_str(), exp.c_str());
  }
  *out = t;
  return VC_OK;
}

int pack_matrix(vc_engine* e, const std::string& key, int N, int Kdim, uint4** out, int th = 16,
                const float* colscale = nullptr) {
  const RawTensor* t;
  int rc = need(e, key, {N, Kdim}, &t);
  if (rc) return rc;
  const int KW = e->dtype == VC_DTYPE_BF16 ? 32 : 16;
  const long units = (long)((N + th - 1) / th) * (Kdim / KW) * 4 * th;
  rc = dalloc(e, out, (size_t)units);
  if (rc) return rc;
  HIPCHK(e, vc_launch_pack(t->dev, colscale, *out, N, Kdim, e->dtype, th, 0));
  return VC_OK;
}

// A linear layer behind a LayerNorm (vc_gemm.hip, "LayerNorm fold"): packs W . gamma, and produces
// wg = rowsum(W . gamma) and the folded bias cb = W beta + bias.
int pack_folded(vc_engine* e, const std::string& wkey, const std::string& bkey, const std::string& ln_prefix,
                int N, int Kdim, uint4** Wout, float** wg, float** cb, int th = 16) {
  const RawTensor *tw, *tb, *tg, *tbe;
  int rc;
  if ((rc = need(e, wkey, {N, Kdim}, &tw))) return rc;
  if ((rc = need(e, bkey, {N}, &tb))) return rc;
  if ((rc = need(e, ln_prefix + "weight", {Kdim}, &tg))) return rc;
  if ((rc = need(e, ln_prefix + "bias", {Kdim}, &tbe))) return rc;
  if ((rc = pack_matrix(e, wkey, N, Kdim, Wout, th, tg->dev))) return rc;
  if ((rc = dalloc(e, wg, (size_t)N))) return rc;
  if ((rc = dalloc(e, cb, (size_t)N))) return rc;
  HIPCHK(e, vc_launch_fold_vecs(tw->dev, tg->dev, tbe->dev, tb->dev, *wg, *cb, N, Kdim, e->dtype, 0));
  return VC_OK;
}

// One packed form of an already packed bf16 image into slot `p`: `planes_u4` 16-byte units of codes and `side_words` words of side
// bytes, packed and checked on the device by `launch` (the kind's pack and check kernels; the w8 kinds check with the conversion their
// GEMMs use).  A unit the codes cannot hold (non-zero exponents that span more than the 13-bit codes do, a value off the 8-bit grid:
// `refused` counts fragments, or pairs), or any dword that does not decode to the image's, refuses the matrix for this layer (state 2:
// the planes are dropped, the launch stays on the image).
template <class Launch>
int pack_checked(vc_engine* e, Layer::Packed& p, size_t planes_u4, size_t side_words, Launch launch) {
  if (!e->w13_counts) { int rc = dalloc(e, &e->w13_counts, (size_t)4); if (rc) return rc; }
  const size_t mark = e->allocs.size();
  const double bytes0 = e->bytes_total;
  int rc;
  if ((rc = dalloc(e, &p.planes, planes_u4))) return rc;
  if ((rc = dalloc(e, &p.side, side_words))) return rc;
  HIPCHK(e, launch(p.planes, reinterpret_cast<unsigned char*>(p.side), e->w13_counts));
  unsigned int cnt[2] = {0, 0};
  HIPCHK(e, hipMemcpy(cnt, e->w13_counts, sizeof cnt, hipMemcpyDeviceToHost));
  p.refused = (int)cnt[0];
  if (cnt[0] == 0 && cnt[1] == 0) { p.state = 1; return VC_OK; }
  p.state = 2;
  while (e->allocs.size() > mark) { (void)hipFree(e->allocs.back()); e->allocs.pop_back(); }
  e->bytes_total = bytes0;
  p.planes = nullptr; p.side = nullptr;
  return VC_OK;
}

int keep_vec(vc_engine* e, const std::string& key, int n, float** out, float* mean = nullptr) {
  const RawTensor* t;
  int rc = need(e, key, {n}, &t);
  if (rc) return rc;
  rc = dalloc(e, out, (size_t)n);
  if (rc) return rc;
  HIPCHK(e, hipMemcpy(*out, t->dev, (size_t)n * 4, hipMemcpyDeviceToDevice));
  if (mean) {
    std::vector<float> host((size_t)n);
    HIPCHK(e, hipMemcpy(host.data(), t->dev, (size_t)n * 4, hipMemcpyDeviceToHost));
    double sum = 0.0;
    for (float v : host) sum += v;
    *mean = (float)(sum / n);
  }
  return VC_OK;
}

// ---------------------------------------------------------------- one forward pass
GemmArgs base_args(vc_engine* e, const RowSrc& rs, const Plan& p, int N, int Kdim) {
  GemmArgs g;
  memset(&g, 0, sizeof g);
  g.N = N; g.K = Kdim; g.n_tiles = p.n_tiles; g.KT = p.KT; g.nchunk = p.nchunk;
  g.r_lds = std::min(rs.n_rows, VC_ROWS);
  g.rows_cap = VC_SLAB_ROWS;
  g.row_seq = rs.row_seq; g.row_pos = rs.row_pos; g.n_rows = rs.n_rows;
  g.n_active = rs.n_active ? rs.n_active : e->one;
  g.nt = (rs.n_active != nullptr || rs.nt) ? 1 : 0;   // decode steps (and the kernel microbenchmarks) stream once; per matrix: nt_bit
  g.d = e->d; g.H = e->H; g.hd = e->hd; g.S_max = e->S_max;
  g.hd_shift = e->hd == 32 ? 5 : e->hd == 64 ? 6 : 7;            // head_dim is 32, 64 or 128 (vc_create)
  g.cache_seq_stride = (long)e->H * e->S_max * e->hd;
  g.dbg_ts = e->dbg_ts;
  g.row_mu = e->mu_zero;
  g.wd_stage = e->wd_stage;
  return g;
}

inline int attn_nt_for(const vc_engine* e, int rows) { return e->attn_nt == 1 || (e->attn_nt == 2 && rows >= 2); }
enum { NT_QKV = 1, NT_O = 2, NT_F1 = 4, NT_F2 = 8, NT_H1 = 16, NT_H2 = 32 };
inline void nt_bit(const vc_engine* e, GemmArgs& g, int bit) { if (!(e->nt_decode & bit)) g.nt = 0; }

int attn_nsplit(const vc_engine* e, int rows) {
  // 8-wave blocks: one decode row is covered by ~256 of them; several rows get ~512 (two per CU), which
  // halves the positions each block walks while the merge in the out-projection stays <= 4 partials
  int ns = (rows > 1 ? e->attn_blocks_multi : e->attn_blocks_one) / std::max(1, rows * e->H);   // (fewer splits = a cheaper merge in the out-projection)
  return std::max(1, std::min(ns, VC_MAX_NSPLIT));
}

// Rows a pass may carry in the finished-row form: X of the FFN down-projection (rows x 4d elements) has to fit the LDS
// of one workgroup, and the out-projection merges rows x nsplit <= 16 attention partials per thread in one batch.
int fr_max_rows(const vc_engine* e) {
  // the FFN down-projection decides (X = rows x 4d elements): one piece up to 8 rows in bf16 at d = 2048 (4 in the exact mode), two
  // halves beyond while a wave can hold its fragments of both; vc_gemm_fr_form is the launcher's own statement of that
  int r = std::min(e->fr_rows, VC_ROWS);
  while (r >= 2 && vc_gemm_fr_form(r, e->d, 4 * e->d, e->dtype, PRO_PLAIN, 1) == 0) --r;
  return r >= 2 ? r : 0;
}

// K slices of a split-K producer on the wide-decode kernel (rows_gemm_wd_k: two 16-channel tiles per workgroup, the slice split over
// 8 waves): the fewest slices that put a workgroup on every CU, among those the kernel has a form for; 0 = none.
int wd_ksplit(const vc_engine* e, int N, int Kdim) {
  const int n_wg = (N / 16 + 1) / 2;
  int best = 0;
  for (int ks = 1; ks <= VC_MAX_KSPLIT; ks *= 2) {
    if (!vc_gemm_wd_kpw(Kdim, e->dtype, ks)) continue;
    best = ks;
    if (n_wg * ks >= 256) break;
  }
  return best;
}

// The forms of a pass.  Slab: 1 row, and 3..16 rows where the finished-row form cannot run - the producers leave split-K slabs that
// the next LayerNorm sums.  Finished rows (2..fr_max_rows rows): five launches per layer, no slabs, no LayerNorm launch - QKV and
// FFN-up fold the LayerNorm of whole rows (PRO_LNW / PRO_LNQ), the out-projection and FFN-down own 8 output channels over the whole K
// and add residual + bias (rows_gemm_fr_k).  Wide: decode steps of 17..64 rows, weight streams on rows_gemm_wd_k / rows_gemm_mt_k.
// Block: prefill passes of more rows, the MFMA block GEMM.  Wide and block passes normalise every row in ln_rows_k.
enum { FORM_SLAB = 0, FORM_FR = 1, FORM_WIDE = 2, FORM_BLOCK = 3 };   // (values: vc_debug_plan out[1])
enum { ATT_ROWS = 0, ATT_TILE = 1, ATT_TILE64 = 2 };                 // rows_attn_k, tile_attn_k, tile_attn64_k
// The in-GEMM LayerNorm prologue walks the rows one after the other (each a dependent round trip in every one of the 384-512
// workgroups): from this many rows on, a per-row LayerNorm launch plus the plain prologue is cheaper (8 rows 20 us -> ~12 us per GEMM).
constexpr int ln_split_rows = 3;

}  // namespace
namespace vch __attribute__((visibility("hidden"))) {
// decode: a decode step (n_active set).  tiled: a prefill pass whose 16-row tiles (1) or 64-row blocks (2) each hold consecutive
// positions of ONE sequence (prefill_batch): MFMA attention; 0 for passes of up to VC_ROWS rows.
PassPlan plan_pass(const vc_engine* e, int rows, bool decode, int tiled) {
  PassPlan p{};
  const int d = e->d;
  const bool bf16 = e->dtype == VC_DTYPE_BF16;
  if (rows <= VC_ROWS && !tiled) p.form = rows >= 2 && rows <= fr_max_rows(e) ? FORM_FR : FORM_SLAB;
  else p.form = decode && rows <= VC_MAX_SEQS ? FORM_WIDE : FORM_BLOCK;
  p.attn = p.form == FORM_BLOCK && tiled ? (tiled == 2 ? ATT_TILE64 : ATT_TILE) : ATT_ROWS;
  p.ks_o = e->p_o.ksplit; p.ks_f2 = e->p_f2.ksplit;
  if (p.form == FORM_SLAB) {
    p.nsplit = attn_nsplit(e, rows);
    p.ln_launch = rows >= ln_split_rows;
    // one row, option fr_one: the FFN down-projection writes the FINISHED residual row into hB (row_gemm_fr1_k), so the row entering a
    // layer is whole: the QKV prologue reads it alone and writes nothing, the FFN-up prologue adds the out-projection's two slabs to it
    // and leaves h' in hA for the down-projection's epilogue.  (The first build - FFN-down alone - gained 2.1 % at giga830M and LOST
    // 1.5 % at giga330M, whose d / 8 = 128 workgroups fill half the chip; together with the paired QKV projection it takes along the
    // form gains there too: -0.5 % +- 0.1 / -0.9 % +- 0.09 on two boxes, profiles/r05e_ab_330M.log, r05f_ab_330M.log.)
    p.fd = rows == 1 && e->fr_one && e->has_fr8 && vc_gemm_fr1_ok(d, 4 * d, e->dtype, VC_FR_WAVES);
    p.qkv_fr1 = p.fd && e->qkv_p8 && e->has_qkv8 && !p.ln_launch;
  } else if (p.form == FORM_FR) {
    // splits of the decode attention: the out-projection merges rows x splits <= 16 partials per thread in one batch of loads; past
    // VC_FR_MAX_ROWS rows the attention is unsplit (rows x heads >= 144 workgroups) and normalises itself (unsplit from 5 rows measured
    // +1.7..+4.5 %, r04j)
    if (rows > VC_FR_MAX_ROWS) {
      p.nsplit = 1;
    } else {
      const int ns = std::min(attn_nsplit(e, rows), 16 / rows);
      p.nsplit = 1;
      while (p.nsplit * 2 <= ns) p.nsplit *= 2;
      p.nsplit = std::max(2, p.nsplit);
    }
    p.att_x = p.nsplit == 1;
    p.part16 = e->att_p16 && bf16 && p.nsplit > 1;
    // the centred copy when a row of it is whole 1 KB requests of a wave (64 lanes x 16 bytes: d a multiple of 512 in bf16, of 256 in
    // fp32); other widths keep the fp32 rows
    const int row_bytes = d * (bf16 ? 2 : 4);
    p.hq = e->hq != 0 && row_bytes % 1024 == 0 && row_bytes <= 8192;
    // weight tiles per consumer workgroup: two from 5 rows up (8 rows -3.4 % +- 0.1, 4 rows +0.5 % +- 0.05, profiles/r04b_bench_batch*),
    // and two rows per wave past VC_FR_MAX_ROWS
    p.mt = rows > VC_FR_MAX_ROWS ? 4 : rows >= 5 ? 3 : 0;
    // the 8-channel QKV image behind a centred copy (profiles/r06i_ab_qp.log, per step: giga830M 2 / 4 / 6 / 8 rows -2.0 / -1.1 / -0.3 /
    // +0.5 %, giga330M 8 rows -1.3 %): at d >= 2048 the form stops at 6 rows (the 8-row launch itself: 7.42 us against 7.33 us)
    p.qp = e->qkv_p8 >= 2 && p.hq && e->has_qkv8 && rows <= (d >= 2048 ? 6 : 8) && vc_gemm_qp_ok(rows, 3 * d, d, e->dtype) != 0;
    p.frp = e->fr_pair && vc_gemm_frp_ok(rows, d, 4 * d, e->dtype);
    // option "w8r": the two paired launches on the E4M3 bytes, where the launcher has a form for these rows (a wave's fragments per
    // tile whole groups: FFN-down at d = 512 / 1024 / 2048, QKV at d = 2048).  The sites take it for the layers whose matrix is packed.
    const vc_packed_kind& pk8 = vc_packed(VC_PK_W8);
    p.frp_w8 = p.frp && (e->w8r & W8_BITS[W13_F2]) && w8_rows_win(W8F_ROWS, rows) && pk8.frp_ng(rows, d, 4 * d, e->dtype) != 0;
    p.qp_w8 = p.qp && (e->w8r & W8_BITS[W13_QKV]) && w8_rows_win(W8F_ROWS, rows) && pk8.qp_ng(rows, 3 * d, d, e->dtype) != 0;
    // option "w8m": past 8 rows the paired producer stops (vc_gemm_frp_ok) and FFN-down runs on rows_gemm_fr_k / rows_gemm_fr2_k; their
    // w8 twins where a wave's k-tiles per piece are whole groups (d = 512 / 1024 / 2048).  The site takes it for the layers whose
    // matrix is packed.
    p.fr_w8_f2 = !p.frp && rows > VC_FR_MAX_ROWS && rows <= VC_ROWS && (e->w8m & W8_BITS[W13_F2]) && pk8.fr_ng(rows, d, 4 * d, e->dtype) != 0 &&
                 (w8_rows_win(W8F_MID, rows) || (e->w8m & 8));
    // option "w8ur": the FFN up-projection behind a centred copy on the pair planes of W1, where the launcher has a form for these rows
    // (K = d in one chunk of 4, 8 or 16 k-tiles per wave: d = 512 / 1024 / 2048).  The site takes it for the layers whose W1 is packed.
    p.lnq_w8_f1 = p.hq && (e->w8ur & W8_BITS[W13_F1]) && pk8.lnq_ok(rows, 4 * d, d, e->dtype) != 0 && (w8_rows_win(W8F_UP_ROWS, rows) || (e->w8ur & 8));
    // option "w8q": the QKV projection behind a centred copy on the pairs of the 12-channel image, at the row counts the paired consumer
    // leaves to rows_gemm_k (p.qp covers 2..6 rows at d = 2048 and 2..8 at narrower widths; with qkv_p8 < 2 none) and where the launcher
    // has a form (K = d in one chunk of 4, 8 or 16 k-tiles per wave).  The site takes it for the layers 1.. whose Wqkv is packed.
    p.qkvq_w8 = p.hq && !p.qp && (e->w8q & W8_BITS[W13_QKV]) && pk8.qkvq_ok(rows, 3 * d, d, e->dtype) != 0 && (w8_rows_win(W8F_QKV_ROWS, rows) || (e->w8q & 8));
  } else {
    p.nsplit = 1;                      // attention one workgroup per (row, head), no split partials
    p.att_x = true;
    p.ln_launch = true;
    p.mt = p.form == FORM_WIDE ? 2 : 1;
    // The 16-channel QKV image has 3/4 of the 12-channel image's tiles, and the block GEMM picks its workgroup tile from the tile count
    // (vc_gemm_pf.hip launch_blk_e: 128-channel tiles from 240 workgroups): where the smaller count would push a pass back to the
    // 64-channel form the 12-channel image stays (giga830M, 385..512 rows: 24.0 us against 34.0, profiles/r05j_qkv16_probe.log);
    // everywhere else the full fragments win or tie (240 rows -6.7 %, 800 rows -1.7 %, 1 280 rows -26.7 %, 32-row decode steps -1.8 %).
    const long blk = (rows + 127) / 128;
    const bool tiles_ok = !((long)(e->p_qkv.n_tiles / 8) * blk >= 240 && (long)(e->p_qkv16.n_tiles / 8) * blk < 240);
    p.qkv16 = e->qkv16 && e->has_qkv16 && (p.form == FORM_WIDE || tiles_ok);
    if (p.form == FORM_WIDE && e->wide_gemm && p.qkv16) {      // every matrix of the layer needs a form on rows_gemm_wd_k
      const int ko = wd_ksplit(e, d, d), kf = wd_ksplit(e, d, 4 * d);
      p.wd = vc_gemm_wd_kpw(d, e->dtype, 1) && ko && kf && vc_gemm_wd_kpw(e->P, e->dtype, 1);
      if (p.wd) { p.ks_o = ko; p.ks_f2 = kf; }
      // option "w8w": FFN-down (on its split-K slices) and QKV on the pair planes, where the staged form runs and the launcher has
      // a form for the slice.  The sites take it for the layers whose matrix is packed.
      const vc_packed_kind& pk8 = vc_packed(VC_PK_W8);
      const bool staged = p.wd && e->wd_stage;
      p.wd_w8_f2 = staged && (e->w8w & W8_BITS[W13_F2]) && pk8.wd_ok(4 * d, e->dtype, p.ks_f2) != 0 &&
                   (w8_rows_win(W8F_WIDE, rows) || (e->w8w & 8));
      p.wd_w8_qkv = staged && (e->w8w & W8_BITS[W13_QKV]) && pk8.wd_ok(d, e->dtype, 1) != 0 &&
                    (w8_rows_win(W8F_WIDE, rows) || (e->w8w & 8));
      // option "w8u": the FFN up-projection likewise (K = d in one slice, as QKV), for the layers whose W1 is packed
      p.wd_w8_f1 = staged && (e->w8u & W8_BITS[W13_F1]) && pk8.wd_ok(d, e->dtype, 1) != 0 && (w8_rows_win(W8F_UP, rows) || (e->w8u & 8));
    }
  }
  p.heads_wide = p.form == FORM_WIDE && e->wide_heads;
  p.heads_fold = p.form == FORM_FR && rows <= VC_FR_MAX_ROWS;
  return p;
}
}  // namespace vch
namespace {

// The rows a LayerNorm reads (a launch, or a GEMM prologue): h_in + prev_bias + n_parts split-K slabs; their sum goes to h_out (may be null).
struct Resid { const float* h_in; float* h_out; int n_parts; const float* prev_bias; };
void set_resid(vc_engine* e, GemmArgs& g, const Resid& r) {
  g.h_in = r.h_in; g.h_out = r.h_out; g.parts = e->parts; g.n_parts = r.n_parts;
  g.prev_bias = r.prev_bias; g.has_prev_bias = r.n_parts > 0 ? 1 : 0;      // (prev_bias: any readable [d] vector when unused)
}
// In front of QKV: h = the residual entering the layer, prev = the layer before (null: layer 0, no slabs).  Behind a finished row the
// prologue reads it alone and writes nothing.
Resid qkv_in(vc_engine* e, const PassPlan& p, const Layer& ly, const float* h, const Layer* prev) {
  return {h, p.fd ? nullptr : e->hA, prev && !p.fd ? p.ks_f2 : 0, prev ? prev->b2 : ly.bo};
}
// In front of FFN-up: h + bo + the out-projection's slabs.
Resid ffn_in(vc_engine* e, const PassPlan& p, const Layer& ly, const float* h) {
  return p.fd ? Resid{h, e->hA, p.ks_o, ly.bo} : Resid{e->hA, e->hB, p.ks_o, ly.bo};
}

// ---- the launch sites of a layer.  h = the residual entering the layer.
int site_ln(vc_engine* e, const RowSrc& rs, const Resid& r, hipStream_t s) {
  GemmArgs g = base_args(e, rs, e->p_f1, 4 * e->d, e->d);
  set_resid(e, g, r);
  g.x_out = e->xn;
  HIPCHK(e, vc_launch_ln_rows(g, e->dtype, s));
  return VC_OK;
}

// The one-row paired launch of matrix `which` of a layer (g.Wp = its image): on the E4M3 bytes where option "w8" has the matrix's bit and
// the matrix is packed that way, else on the 13-bit planes by the same rule for option "w13", else on the image.
hipError_t launch_fr1(const vc_engine* e, const Layer& ly, int which, const GemmArgs& g, int pro, int epi, hipStream_t s) {
  const int mask[VC_PK_N] = {e->w13, e->w8};
  for (int kind = VC_PK_N - 1; kind >= 0; --kind) {      // the w8 bit wins
    const Layer::Packed& p = ly.packed[kind][which];
    if ((mask[kind] & W8_BITS[which]) && p.state == 1) return vc_packed(kind).row(g, p.planes, p.side, pro, epi, s);
  }
  return vc_launch_gemm_fr1(g, e->dtype, pro, epi, s);
}

// The finished-row consumers' `row_mu` ping-pong: QKV reads the means in row_mu[0] and leaves the rows' new means in row_mu[1], which
// the out-projection centres its copy on; FFN-up reads row_mu[1] and leaves row_mu[0] for the FFN down-projection and the heads.
// q,k,v = Wqkv LN1(h) + b ; K/V go straight into the cache.  first: layer 0 (no centred copy of its input rows).
int site_qkv(vc_engine* e, const PassPlan& p, const RowSrc& rs, const Layer& ly, const Resid& r, const Layer* prev, hipStream_t s) {
  const bool first = prev == nullptr;
  const int d = e->d;
  GemmArgs g = base_args(e, rs, e->p_qkv, 3 * d, d);
  g.Wp = ly.Wqkv; nt_bit(e, g, NT_QKV); g.bias = ly.bqkv; g.wg = ly.wg_qkv;
  g.q_out = e->q; g.kcache = ly.kc; g.vcache = ly.vc; g.mt = p.mt;
  if (p.form == FORM_FR) {
    g.h_in = r.h_in;
    if (p.hq) g.row_mu_out = e->row_mu[1];
    if (p.hq && !first) {      // the previous layer's FFN down-projection left hqB = WT(hB - row_mu[0])
      g.x_in = e->hqB; g.x_ld = d; g.row_mu = e->row_mu[0]; g.mu_shift = prev->b2_mean;
      const Layer::Packed& p8 = ly.packed[VC_PK_W8][W13_QKV];
      if (p.qp_w8 && p8.state == 1) { g.Wp = ly.Wqkv8; HIPCHK(e, vc_packed(VC_PK_W8).qp(g, p8.planes, p8.side, s)); }
      else if (p.qp) { g.Wp = ly.Wqkv8; HIPCHK(e, vc_launch_gemm_qp(g, e->dtype, s)); }
      else if (p.qkvq_w8 && ly.w8q.state == 1)      // ... on the pairs of the 12-channel image (a refused layer keeps its image)
        HIPCHK(e, vc_packed(VC_PK_W8).qkvq(g, ly.w8q.planes, reinterpret_cast<const uint8_t*>(ly.w8q.side), s));
      else HIPCHK(e, vc_launch_gemm(g, e->dtype, PRO_LNQ, EPI_QKV, 1, 1, s));
    } else {
      HIPCHK(e, vc_launch_gemm(g, e->dtype, PRO_LNW, EPI_QKV, 1, 1, s));
    }
    return VC_OK;
  }
  set_resid(e, g, r);
  if (p.qkv_fr1) {         // the row entering the layer is finished (layer 0: the sampler's dec_h row): 8-channel tiles, two k-tiles per fragment
    g.Wp = ly.Wqkv8;
    HIPCHK(e, launch_fr1(e, ly, W13_QKV, g, PRO_LN, EPI_QKV, s));
  } else if (!p.ln_launch) {
    HIPCHK(e, vc_launch_gemm(g, e->dtype, PRO_LN, EPI_QKV, 1, 1, s));
  } else if (p.qkv16) {    // every A lane a weight: the 16-channel image
    g.x_in = e->xn; g.x_ld = d;
    g.Wp = ly.Wqkv16; g.n_tiles = e->p_qkv16.n_tiles; g.KT = e->p_qkv16.KT; g.nchunk = e->p_qkv16.nchunk;
    const Layer::Packed& pw = ly.packed[PK_W8W][W13_QKV];
    if (p.wd_w8_qkv && pw.state == 1)      // ... on the pair planes (a refused layer keeps its image)
      HIPCHK(e, vc_packed(VC_PK_W8).wd(g, pw.planes, reinterpret_cast<const uint8_t*>(pw.side), EPI_QKV16, 1, s));
    else if (p.wd) HIPCHK(e, vc_launch_gemm_wd(g, e->dtype, EPI_QKV16, 1, 1, s));
    else HIPCHK(e, vc_launch_gemm(g, e->dtype, PRO_PLAIN, EPI_QKV16, 1, 1, s));
  } else {
    g.x_in = e->xn; g.x_ld = d;
    HIPCHK(e, vc_launch_gemm(g, e->dtype, PRO_PLAIN, EPI_QKV, 1, 1, s));
  }
  return VC_OK;
}

// What options "kv8" / "kv8c" add to a pass, decided in ONE place (site_attn and run_pass follow it, vc_debug_kv8_plan reports it):
// the form of the rows_attn_k launches (VC_KV8_ATTN_*) and the launches queued behind the last layer, in order (VC_KV8_LAUNCH_*).
// request: 0 no request, 1 vc_request_kv8, 2 vc_request_kv8c; kv8: the option's value; rps: rows per sequence of a decode pass, 0 for a
// prefill pass; rows_attn: the pass's attention is rows_attn_k (not a tile kernel).
struct Kv8Plan { int attn; int n_tail; int tail[2]; };
Kv8Plan kv8_plan(int request, int kv8, int rps, bool rows_attn) {
  Kv8Plan k = {VC_KV8_ATTN_PLAIN, 0, {0, 0}};
  if (request <= 0) return k;                                  // nothing more is allocated or launched
  const bool centred = request >= 2;
  // decode passes read the positions older than the pass from the E4M3 cache; prefill passes and option 0 stay on the bf16 cache
  if (kv8 && rps > 0 && rows_attn) k.attn = centred ? VC_KV8_ATTN_CENTRED : VC_KV8_ATTN_E4M3;
  // a prefill pass of a centred engine leaves the centres of the slots whose position 0 it holds, in front of the packer
  if (centred && rps == 0) k.tail[k.n_tail++] = VC_KV8_LAUNCH_CENTRE;
  // the rows the pass wrote, as E4M3 bytes too - prefill and decode passes alike, whatever the option's value
  k.tail[k.n_tail++] = centred ? VC_KV8_LAUNCH_PACK_CENTRED : VC_KV8_LAUNCH_PACK;
  return k;
}
Kv8Plan kv8_plan(const vc_engine* e, const PassPlan& p, const RowSrc& rs) {
  return kv8_plan(e->kv8c_req ? 2 : e->kv8_req ? 1 : 0, e->kv8, rs.rps, p.attn == ATT_ROWS);
}

int site_attn(vc_engine* e, const PassPlan& p, const RowSrc& rs, const Layer& ly, hipStream_t s) {
  AttnArgs a;
  memset(&a, 0, sizeof a);
  a.q = e->q; a.kcache = ly.kc; a.vcache = ly.vc;
  a.cache_seq_stride = (long)e->H * e->S_max * e->hd;
  a.S_max = e->S_max; a.H = e->H; a.hd = e->hd; a.hd_shift = e->hd == 32 ? 5 : e->hd == 64 ? 6 : 7; a.d = e->d; a.nsplit = p.nsplit;
  a.scale = 1.0f / sqrtf((float)e->hd);
  a.row_seq = rs.row_seq; a.row_pos = rs.row_pos; a.n_rows = rs.n_rows;
  a.n_active = rs.n_active ? rs.n_active : e->one; a.dbg_ts = e->dbg_ts;
  a.att_o = e->att_o; a.att_ml = e->att_ml; a.share_len = e->share_len;
  a.nt = (rs.n_active != nullptr || rs.nt) ? attn_nt_for(e, rs.n_rows) : 0;   // decode passes stream their K/V once, prefill passes re-read it
  a.fast = e->attn_fast;
  a.part16 = p.part16 ? 1 : 0;
  const int form8 = kv8_plan(e, p, rs).attn;
  if (form8 != VC_KV8_ATTN_PLAIN) {      // decode passes of a kv8 engine: positions older than the pass from the E4M3 cache
    a.kcache8 = ly.kc8; a.vcache8 = ly.vc8; a.kvshift8 = ly.sh8; a.rps = rs.rps;
    if (form8 == VC_KV8_ATTN_CENTRED) a.centre = ly.kcen;
  }
  if (p.att_x) a.x_out = e->xn;        // xn is free between the QKV GEMM and the FFN LayerNorm
  if (p.attn == ATT_TILE64) HIPCHK(e, vc_launch_tile_attn64(a, s));
  else if (p.attn == ATT_TILE) HIPCHK(e, vc_launch_tile_attn(a, e->dtype, s));
  else HIPCHK(e, vc_launch_attn(a, e->dtype, rs.n_rows, s));
  return VC_OK;
}

// h' = h + bo + Wo attn: finished rows into hA, or split-K slabs
int site_oproj(vc_engine* e, const PassPlan& p, const RowSrc& rs, const Layer& ly, const float* h, hipStream_t s) {
  const int d = e->d;
  GemmArgs g = base_args(e, rs, e->p_o, d, d);
  if (p.form == FORM_FR) {
    g.Wp = ly.Wo8; g.bias = ly.bo;
    g.h_in = h; g.h_out = e->hA;
    if (p.hq) { g.hq_out = e->hqA; g.row_mu = e->row_mu[1]; g.mu_shift = ly.bo_mean; }      // centred on the mean the QKV consumer found for h + the mean of bo
    if (p.att_x) {
      g.x_in = e->xn; g.x_ld = d;
      HIPCHK(e, vc_launch_gemm_fr(g, e->dtype, PRO_PLAIN, s));
    } else {
      g.att_o = e->att_o; g.att_ml = e->att_ml; g.nsplit = p.nsplit; g.att_p16 = p.part16 ? 1 : 0;
      HIPCHK(e, vc_launch_gemm_fr(g, e->dtype, PRO_ATT, s));
    }
    return VC_OK;
  }
  g.Wp = ly.Wo; nt_bit(e, g, NT_O); g.part_out = e->parts; g.mt = p.mt;
  if (p.att_x) {
    g.x_in = e->xn; g.x_ld = d;
    if (p.wd) HIPCHK(e, vc_launch_gemm_wd(g, e->dtype, EPI_PART, p.ks_o, 1, s));
    else HIPCHK(e, vc_launch_gemm(g, e->dtype, PRO_PLAIN, EPI_PART, p.ks_o, 1, s));
  } else {                 // merge the attention partials of all heads
    g.att_o = e->att_o; g.att_ml = e->att_ml; g.nsplit = p.nsplit;
    HIPCHK(e, vc_launch_gemm(g, e->dtype, PRO_ATT, EPI_PART, p.ks_o, 1, s));
  }
  return VC_OK;
}

// a = relu(W1 LN2(h') + b1)
int site_ffn_up(vc_engine* e, const PassPlan& p, const RowSrc& rs, const Layer& ly, const Resid& r, hipStream_t s) {
  const int d = e->d;
  GemmArgs g = base_args(e, rs, e->p_f1, 4 * d, d);
  g.Wp = ly.W1; nt_bit(e, g, NT_F1); g.bias = ly.b1; g.wg = ly.wg_1;
  g.out = e->act; g.out_ld = 4 * d; g.mt = p.mt;
  if (p.form == FORM_FR) {
    g.h_in = r.h_in;
    if (p.hq) {
      g.x_in = e->hqA; g.x_ld = d; g.row_mu = e->row_mu[1]; g.mu_shift = ly.bo_mean; g.row_mu_out = e->row_mu[0];
      const Layer::Packed& pw = ly.packed[PK_W8W][W13_F1];
      if (p.lnq_w8_f1 && pw.state == 1)      // ... on the pair planes (a refused layer keeps its image)
        HIPCHK(e, vc_packed(VC_PK_W8).lnq(g, pw.planes, reinterpret_cast<const uint8_t*>(pw.side), s));
      else HIPCHK(e, vc_launch_gemm(g, e->dtype, PRO_LNQ, EPI_RELU, 1, 1, s));
    } else {
      HIPCHK(e, vc_launch_gemm(g, e->dtype, PRO_LNW, EPI_RELU, 1, 1, s));
    }
    return VC_OK;
  }
  set_resid(e, g, r);
  if (!p.ln_launch) {
    HIPCHK(e, vc_launch_gemm(g, e->dtype, PRO_LN, EPI_RELU, 1, 1, s));
    return VC_OK;
  }
  g.x_in = e->xn; g.x_ld = d;
  const Layer::Packed& pw = ly.packed[PK_W8W][W13_F1];
  if (p.wd_w8_f1 && pw.state == 1)         // ... on the pair planes (a refused layer keeps its image)
    HIPCHK(e, vc_packed(VC_PK_W8).wd(g, pw.planes, reinterpret_cast<const uint8_t*>(pw.side), EPI_RELU, 1, s));
  else if (p.wd) HIPCHK(e, vc_launch_gemm_wd(g, e->dtype, EPI_RELU, 1, 1, s));
  else HIPCHK(e, vc_launch_gemm(g, e->dtype, PRO_PLAIN, EPI_RELU, 1, 1, s));
  return VC_OK;
}

// h'' = h' + b2 + W2 a: finished rows into hB, or split-K slabs folded into the next LayerNorm together with b2
int site_ffn_down(vc_engine* e, const PassPlan& p, const RowSrc& rs, const Layer& ly, hipStream_t s) {
  const int d = e->d;
  GemmArgs g = base_args(e, rs, e->p_f2, d, 4 * d);
  g.x_in = e->act; g.x_ld = 4 * d;
  if (p.form == FORM_FR || p.fd) {
    g.Wp = ly.W28; g.bias = ly.b2;
    g.h_in = e->hA; g.h_out = e->hB;
    if (p.hq) { g.hq_out = e->hqB; g.row_mu = e->row_mu[0]; g.mu_shift = ly.b2_mean; }      // centred on the mean the FFN-up consumer found for h' + the mean of b2
    if (p.fd) HIPCHK(e, launch_fr1(e, ly, W13_F2, g, PRO_PLAIN, EPI_RES, s));
    else if (p.frp_w8 && ly.packed[VC_PK_W8][W13_F2].state == 1)        // ... on the E4M3 bytes (a refused matrix keeps its image)
      HIPCHK(e, vc_packed(VC_PK_W8).frp(g, ly.packed[VC_PK_W8][W13_F2].planes, ly.packed[VC_PK_W8][W13_F2].side, s));
    else if (p.frp) HIPCHK(e, vc_launch_gemm_frp(g, e->dtype, s));      // 2..8 rows: two k-tiles per fragment
    else if (p.fr_w8_f2 && ly.packed[VC_PK_W8][W13_F2].state == 1)      // 9..16 rows on the E4M3 bytes (a refused matrix keeps its image)
      HIPCHK(e, vc_packed(VC_PK_W8).fr(g, ly.packed[VC_PK_W8][W13_F2].planes, ly.packed[VC_PK_W8][W13_F2].side, s));
    else HIPCHK(e, vc_launch_gemm_fr(g, e->dtype, PRO_PLAIN, s));
    return VC_OK;
  }
  g.Wp = ly.W2; nt_bit(e, g, NT_F2); g.part_out = e->parts; g.mt = p.mt;
  const Layer::Packed& pw = ly.packed[PK_W8W][W13_F2];
  if (p.wd_w8_f2 && pw.state == 1)         // ... on the pair planes (a refused layer keeps its image)
    HIPCHK(e, vc_packed(VC_PK_W8).wd(g, pw.planes, reinterpret_cast<const uint8_t*>(pw.side), EPI_PART, p.ks_f2, s));
  else if (p.wd) HIPCHK(e, vc_launch_gemm_wd(g, e->dtype, EPI_PART, p.ks_f2, 1, s));
  else HIPCHK(e, vc_launch_gemm(g, e->dtype, PRO_PLAIN, EPI_PART, p.ks_f2, 1, s));
  return VC_OK;
}

}  // namespace
namespace vch __attribute__((visibility("hidden"))) {
// One pass of rs.n_rows rows through every layer, in the form `p` plans.
int run_pass(vc_engine* e, const PassPlan& p, const RowSrc& rs, PassOut* out, hipStream_t s) {
  for (int l = 0; l < e->L; ++l) {
    const Layer& ly = e->layers[l];
    const Layer* prev = l > 0 ? &e->layers[l - 1] : nullptr;
    const float* h = prev ? e->hB : rs.h_in;
    const Resid rq = qkv_in(e, p, ly, h, prev), rf = ffn_in(e, p, ly, h);
    int rc;
    if ((p.ln_launch && (rc = site_ln(e, rs, rq, s))) || (rc = site_qkv(e, p, rs, ly, rq, prev, s)) || (rc = site_attn(e, p, rs, ly, s)) ||
        (rc = site_oproj(e, p, rs, ly, h, s)) || (p.ln_launch && (rc = site_ln(e, rs, rf, s))) || (rc = site_ffn_up(e, p, rs, ly, rf, s)) ||
        (rc = site_ffn_down(e, p, rs, ly, s)))
      return rc;
  }
  const bool finished = p.form == FORM_FR || p.fd;
  *out = {finished ? 0 : p.ks_f2, p.hq ? e->hqB : nullptr, e->row_mu[0]};
  const Kv8Plan k8 = kv8_plan(e, p, rs);      // options "kv8" / "kv8c": the launches behind the last layer, in the plan's order
  for (int i = 0; i < k8.n_tail; ++i) {
    Kv8PackArgs k;
    memset(&k, 0, sizeof k);
    k.layers = e->kv8_tab; k.L = e->L; k.H = e->H; k.hd = e->hd; k.hd_shift = e->hd == 32 ? 5 : e->hd == 64 ? 6 : 7; k.S_max = e->S_max;
    k.row_seq = rs.row_seq; k.row_pos = rs.row_pos; k.n_rows = rs.n_rows; k.n_active = rs.n_active ? rs.n_active : e->one;
    if (k8.tail[i] == VC_KV8_LAUNCH_CENTRE) {
      Kv8CentreArgs c;
      memset(&c, 0, sizeof c);
      c.layers = e->kv8_tab; c.centres = e->kcen_tab; c.n0 = e->kcen_rows;
      c.L = k.L; c.H = k.H; c.hd = k.hd; c.hd_shift = k.hd_shift; c.S_max = k.S_max; c.n_slots = e->B_max;
      c.row_seq = k.row_seq; c.row_pos = k.row_pos; c.n_rows = k.n_rows; c.n_active = k.n_active; c.share_len = e->share_len;
      HIPCHK(e, vc_launch_kv8c_centre(c, s));
      continue;
    }
    if (k8.tail[i] == VC_KV8_LAUNCH_PACK_CENTRED) k.centres = e->kcen_tab;
    HIPCHK(e, vc_launch_kv8_pack(k, s));
  }
  return VC_OK;
}
}  // namespace vch
namespace {

// final LayerNorm + heads-1 for n rows; row r reads hidden row gather[r] (or in_row0 + r) and writes hh row (out_row0 + r).  wide: all
// rows of a 17..64-row step at once on the weight-stationary kernel of those steps (LayerNorm launch + rows_gemm_wd_k / rows_gemm_mt_k)
int site_heads1(vc_engine* e, const PassPlan& p, const PassOut& po, bool wide, const int* gather, int n, int in_row0, int out_row0,
                const int* n_active, hipStream_t s) {
  if (gather && n > 1) return fail(e, VC_EINVAL, "internal: a gathered head pass carries one row");
  RowSrc rs{};
  rs.n_rows = n; rs.n_active = n_active;
  const int d = e->d;
  GemmArgs g = base_args(e, rs, e->p_h1, e->K * e->P, d);
  g.Wp = e->Wh1; nt_bit(e, g, NT_H1); g.bias = e->bh1; g.wg = e->wg_h1; g.gather_rows = gather;
  g.h_in = e->hB + (size_t)in_row0 * d; g.parts = e->parts + (size_t)in_row0 * d; g.n_parts = po.n_parts;
  g.prev_bias = e->layers[e->L - 1].b2; g.has_prev_bias = po.n_parts > 0 ? 1 : 0;
  g.out = (char*)e->hh + (size_t)out_row0 * e->K * e->P * e->esz; g.out_ld = e->K * e->P;
  if (p.heads_fold && !gather) {                  // finished rows: LayerNorm fold per wave, no extra launch
    if (po.hq && in_row0 == 0) {                  // ... on the last FFN down-projection's centred copy
      g.x_in = po.hq; g.x_ld = d; g.row_mu = po.mu;
      HIPCHK(e, vc_launch_gemm(g, e->dtype, PRO_LNQ, EPI_GELU, 1, 1, s));
    } else {
      HIPCHK(e, vc_launch_gemm(g, e->dtype, PRO_LNW, EPI_GELU, 1, 1, s));
    }
  } else if (!gather && n >= ln_split_rows) {      // (wide: always)
    g.x_out = e->xn;
    HIPCHK(e, vc_launch_ln_rows(g, e->dtype, s));
    g.x_in = e->xn; g.x_ld = d;
    if (wide) g.mt = 2;
    if (wide && p.wd) HIPCHK(e, vc_launch_gemm_wd(g, e->dtype, EPI_GELU, 1, 1, s));
    else HIPCHK(e, vc_launch_gemm(g, e->dtype, PRO_PLAIN, EPI_GELU, 1, 1, s));
  } else {
    HIPCHK(e, vc_launch_gemm(g, e->dtype, PRO_LN, EPI_GELU, 1, 1, s));
  }
  return VC_OK;
}
// heads-2: the K codebook logits of hh rows out_row0.. (one group per codebook)
int site_heads2(vc_engine* e, const PassPlan& p, bool wide, int n, int out_row0, const int* n_active, hipStream_t s) {
  RowSrc rs{};
  rs.n_rows = n; rs.n_active = n_active;
  GemmArgs g = base_args(e, rs, e->p_h2, e->V, e->P);
  g.Wp = e->Wh2; nt_bit(e, g, NT_H2); g.bias = e->bh2;
  g.w_group_stride = e->wh2_group_stride; g.bias_group_stride = e->V;
  g.x_in = (char*)e->hh + (size_t)out_row0 * e->K * e->P * e->esz; g.x_ld = e->K * e->P; g.x_group_stride = e->P;
  g.out = e->logits + (size_t)out_row0 * e->K * e->V;
  if (wide) g.mt = 2;
  if (wide && p.wd) HIPCHK(e, vc_launch_gemm_wd(g, e->dtype, EPI_LOGITS, 1, e->K, s));
  else HIPCHK(e, vc_launch_gemm(g, e->dtype, PRO_PLAIN, EPI_LOGITS, 1, e->K, s));
  return VC_OK;
}
}  // namespace
namespace vch __attribute__((visibility("hidden"))) {
// The prediction heads (voicecraft.py:181-185, :1084-1086) behind pass `p`: at 17..64 rows once over the step (option wide_heads: the
// 16-row passes streamed the 33.6 MB of head weights four times at 64 rows), otherwise 16 rows at a time.
int run_heads(vc_engine* e, const PassPlan& p, const PassOut& po, const int* gather, int n, int in_row0, int out_row0,
              const int* n_active, hipStream_t s) {
  const bool wide = p.heads_wide && !gather;
  const int step = wide ? n : VC_ROWS;
  for (int r0 = 0; r0 < n; r0 += step) {
    const int m = std::min(step, n - r0);
    int rc;
    if ((rc = site_heads1(e, p, po, wide, gather, m, in_row0 + r0, out_row0 + r0, n_active, s)) ||
        (rc = site_heads2(e, p, wide, m, out_row0 + r0, n_active, s)))
      return rc;
  }
  return VC_OK;
}
}  // namespace vch
namespace {

// Prefill attention of a call whose longest prompt has `longest` rows: 2 = tile_attn64_k on 64-row blocks, 1 = tile_attn_k on 16-row tiles.
// (tile_attn64_k's gain grows with the sequence - 800 rows -15 %, 2048 rows -39 % of the attention launch; 512 rows +8 % -, while the 64-row
// layout costs up to 48 padding rows per prompt in every GEMM of the pass: config 5's eight 231-row prompts would pay 6.7 % more GEMM rows
// for no attention gain (measured neutral: prefill 5.2 ms either way, profiles/r04p_default_attn64.log), so they stay on the first kernel
// and 16-row boundaries.  And only when the passes are cut on 64-row boundaries: with a `prefill_rows` option that is not a multiple of
// 64 a block of a later pass would straddle one prompt's tail padding and the next prompt's first rows - ADVICE r04.)
int prefill_tiled(const vc_engine* e, long longest) {
  const bool attn64 = e->tile_attn == 2 && e->dtype == VC_DTYPE_BF16 && e->hd == 128 && longest >= e->tile_attn_min_rows &&
                      e->prefill_rows_per_pass % 64 == 0;
  return attn64 ? 2 : 1;
}

}  // namespace
namespace vch __attribute__((visibility("hidden"))) {
// Prefill of one or several prompts as ONE row stream: the prompts' rows are laid back to back in `emb`
// (each row carries its own (sequence, position)), pushed through the decoder in passes of up to
// prefill_rows_per_pass rows - so the weights are streamed once per pass for all sequences together, not
// once per sequence - and the heads run on the last row of each prompt as soon as its pass is through.
// pas[i] describes prompt i (x, y, segments); slots[i] is its sequence slot.
// sess: a decode session's admission - the prompts' error bits go to prompt_err[slot] (attributable to a request) and the heads gather
// through sess_gather, so that nothing the live rows of the running batch own is written.
int prefill_batch(vc_engine* e, std::vector<PromptArgs>& pas, const std::vector<int>& slots, hipStream_t s, bool sess) {
  int* const gather = sess ? e->sess_gather : e->logit_row;
  const int chunk = e->prefill_rows_per_pass;
  size_t i0 = 0;
  while (i0 < pas.size()) {
    // ---- a group of prompts that fits the row arena
    // (every prompt starts on a multiple of 16 rows, so that a 16-row tile never mixes sequences: the MFMA
    // attention of the prefill works on such tiles; the padding rows are inactive, row_pos = -1)
    size_t i1 = i0;
    int R = 0;
    // (tile_attn64_k works on 64-row blocks of one sequence: prompts then start on multiples of 64 rows; prefill_tiled)
    long longest = 0;
    for (const PromptArgs& pa : pas) longest = std::max<long>(longest, pa.Lx + pa.n_cols - pa.skip);
    const int tiled = prefill_tiled(e, longest);
    const int al = tiled == 2 ? 64 : 16;
    auto rows_of = [al](const PromptArgs& pa) { return ((pa.Lx + pa.n_cols - pa.skip) + al - 1) & ~(al - 1); };
    while (i1 < pas.size() && (i1 == i0 || R + rows_of(pas[i1]) <= e->emb_cap)) {
      R += rows_of(pas[i1]);
      ++i1;
    }
    if (R > e->emb_cap) return fail(e, VC_ECAP, "a prompt of %d rows does not fit the prefill arena of %d rows", R, e->emb_cap);
    HIPCHK(e, hipMemsetAsync(e->pre_row_pos, 0xFF, (size_t)R * sizeof(int), s));      // -1 everywhere
    HIPCHK(e, hipMemsetAsync(e->pre_row_seq, 0, (size_t)R * sizeof(int), s));
    HIPCHK(e, hipMemsetAsync(e->emb, 0, (size_t)R * e->d * sizeof(float), s));
    std::vector<int> last(i1 - i0);
    int row0 = 0;
    for (size_t i = i0; i < i1; ++i) {
      PromptArgs& pa = pas[i];
      const int rows = pa.Lx + pa.n_cols - pa.skip;
      pa.seq = slots[i]; pa.row0 = row0;
      pa.emb = e->emb; pa.row_seq = e->pre_row_seq; pa.row_pos = e->pre_row_pos; pa.err = sess ? e->prompt_err + slots[i] : e->err_flag;
      last[i - i0] = row0 + rows - 1;
      pa.logit_row = gather + slots[i];
      pa.logit_row_val = last[i - i0] % chunk;            // index of the prompt's last row inside its pass
      HIPCHK(e, vc_launch_prompt(pa, s));
      row0 += (rows + al - 1) & ~(al - 1);
    }
    for (int r0 = 0; r0 < R; r0 += chunk) {
      RowSrc rs{};
      rs.h_in = e->emb + (size_t)r0 * e->d;
      rs.row_seq = e->pre_row_seq + r0; rs.row_pos = e->pre_row_pos + r0;
      rs.n_rows = std::min(chunk, R - r0);
      const PassPlan p = plan_pass(e, rs.n_rows, false, rs.n_rows > VC_ROWS ? tiled : 0);
      PassOut po;
      int rc = run_pass(e, p, rs, &po, s);
      if (rc) return rc;
      for (size_t i = i0; i < i1; ++i)
        if (last[i - i0] >= r0 && last[i - i0] < r0 + rs.n_rows)
          if ((rc = run_heads(e, p, po, gather + slots[i], 1, 0, slots[i], nullptr, s))) return rc;
    }
    i0 = i1;
  }
  return VC_OK;
}

void fill_prompt_common(vc_engine* e, PromptArgs& pa, const int64_t* x, int Lx, const int64_t* y, int T) {
  memset(&pa, 0, sizeof pa);
  pa.x = x; pa.y = y; pa.Lx = Lx; pa.T = T; pa.K = e->K; pa.d = e->d; pa.V = e->V;
  pa.empty_token = e->cfg.empty_token;
  pa.text_emb = e->text_emb; pa.audio_emb = e->audio_emb; pa.mask_emb = e->mask_emb; pa.pe = e->pe;
  pa.alpha_text = e->alpha_text; pa.alpha_audio = e->alpha_audio;
  pa.text_rows = e->cfg.text_rows;
}

// Engine-constant sampler arguments; the per-call values go through e->h_dyn -> e->d_dyn (push_sample_dyn).
SampleArgs make_sample_args(vc_engine* e, int B, int rps) {
  SampleArgs a;
  memset(&a, 0, sizeof a);
  a.logits = e->logits; a.B = B; a.K = e->K; a.V = e->V; a.d = e->d;
  a.empty_token = e->cfg.empty_token; a.gen_stride = e->gen_cap; a.dyn = e->d_dyn;
  a.st = e->st; a.n_active = e->n_active; a.host_active = e->h_flag + HF_ACTIVE; a.host_live = e->h_flag + HF_LIVE0; a.step_ctr = e->step_ctr; a.graph_steps = std::max(1, e->steps_per_graph); a.samp = e->samp;
  a.err = e->err_flag;
  a.gen = e->gen;
  a.rps = rps; a.dec_h = e->dec_h; a.row_seq = e->dec_row_seq; a.row_pos = e->dec_row_pos;
  a.logit_row = e->logit_row;
  a.audio_emb = e->audio_emb; a.mask_emb = e->mask_emb; a.pe = e->pe; a.alpha_audio = e->alpha_audio;
  a.max_positions = e->S_max;
  return a;
}

int push_sample_dyn(vc_engine* e, const vc_sample_cfg* sc, const int64_t* forced, int n_forced, float* logits_out,
                    int logit_steps, int n_seq, hipStream_t s, int n_group) {
  SampleDyn& d = *e->h_dyn;
  memset(&d, 0, sizeof d);
  d.top_k = sc->top_k; d.top_p = sc->top_p; d.temperature = sc->temperature;
  d.stop_repetition = sc->stop_repetition;
  if (sc->n_silence < 0 || sc->n_silence > VC_MAX_SILENCE)
    return fail(e, VC_EINVAL, "n_silence %d outside [0,%d]", sc->n_silence, VC_MAX_SILENCE);
  d.n_silence = sc->n_silence;
  for (int i = 0; i < d.n_silence; ++i) d.silence[i] = sc->silence_tokens[i];
  d.seed = sc->seed;
  d.forced = forced; d.n_forced = forced ? n_forced : 0; d.forced_mode = sc->forced_mode;
  d.logits_out = logits_out; d.logit_steps = logits_out ? logit_steps : 0;
  d.max_steps = e->gen_cap;                               // rows of the gen buffer per sequence
  d.n_seq = n_seq;                                        // sequences of the call (row stride of forced / logits_out)
  d.n_group = n_group;                                    // samples per best-of-N group (advance_phase's keep decision)
  d.dbg_ts = getenv("VC_SAMPLER_TS") ? e->dbg_ts : nullptr;
  d.seed_tab = e->seed_tab; d.retire_rec = e->h_rec; d.batch_id = e->batch_id; d.row_base = e->row_base; d.adm_slot = e->adm_slot;   // (sessions only)
  d.ctl_tab = e->ctl_tab; d.samp_tab = e->samp_tab;
  HIPCHK(e, hipMemcpyAsync(e->d_dyn, e->h_dyn, sizeof(SampleDyn), hipMemcpyHostToDevice, s));
  return VC_OK;
}
}  // namespace vch
namespace {

int decode_step(vc_engine* e, const SampleArgs& sa, int B, int rps, bool grouped, hipStream_t s, bool sess = false) {
  RowSrc rs{};
  rs.h_in = e->dec_h; rs.row_seq = e->dec_row_seq; rs.row_pos = e->dec_row_pos;
  rs.n_rows = B * rps; rs.n_active = e->n_active; rs.rps = rps;
  const PassPlan p = plan_pass(e, rs.n_rows, true, 0);
  PassOut po;
  int rc = run_pass(e, p, rs, &po, s);
  if (rc) return rc;
  // rps == 1: logit_row[b] == b (vc_tokens.hip advance_phase); the 3-row span switch is single-sequence
  rc = run_heads(e, p, po, rps == 1 ? nullptr : e->logit_row, B, 0, 0, e->n_active, s);
  if (rc) return rc;
  if (sess) HIPCHK(e, vc_launch_sample_session(sa, false, B, grouped, s));     // (grouped: a session opened for best-of-N requests)
  else HIPCHK(e, vc_launch_sample(sa, grouped, s));
  return VC_OK;
}

// The decode loop: every step is the same launch sequence (all step-dependent values live in HBM, the
// per-call sampler values behind a pointer), so `steps_per_graph` steps are captured ONCE per (sequences,
// rows per sequence, best-of-N) into a hipGraphExec that is kept for the life of the engine and replayed.
// The host never touches the stream inside the loop: the device clears a pinned host word when the last
// sequence retires, and the host paces itself one graph behind the GPU with events, so a queued graph is
// always waiting when the running one ends (measured before: ~8 us of idle GPU per graph launch and ~100 us
// per blocking poll).  Steps replayed after the last sequence retired are no-ops (*n_active == 0).
void drop_tts_stream(vc_engine* e);

}  // namespace
namespace vch __attribute__((visibility("hidden"))) {
// Rows per step.  A multi-utterance call starts with one row per sequence; when few enough sequences are left (option "shrink") the
// live ones are re-packed onto the rows of a narrower step - the next power of two >= the live count - and the loop goes on with
// that width's captured graph (graphs are keyed by width).  B / sa = the width in force.  Best-of-N calls of two or more groups shrink
// too (a decided group keeps one live row); a call of ONE group does not: its step stays N rows wide, as it always has.
void DecodeLoop::init(vc_engine* e_, const SampleArgs& sa0, int B0_, int rps_, int groups_, const vc_sample_cfg* sc_, int max_steps_, hipStream_t s_) {
  e = e_; sa = sa0; sc = *sc_; B0 = B = B0_; rps = rps_; groups = groups_; max_steps = max_steps_; s = s_;
  G = std::max(1, e->steps_per_graph);
  grouped = groups > 0;
  can_shrink = e->shrink && groups != 1 && rps == 1 && B0 > 1;
  launched = batch = complete = 0; over = false;
}
int DecodeLoop::width_for(int live) { int p = 1; while (p < live) p *= 2; return p; }
// One captured graph per (rows per step, option state), kept for the life of the engine.
int DecodeLoop::exec_for(hipGraphExec_t* out) {
  const auto key = std::make_pair(std::make_tuple(B, rps, sess ? (grouped ? 3 : 2) : grouped ? 1 : 0), e->opt_state);
  auto it = e->graphs.find(key);
  int rc = VC_OK;
  if (it != e->graphs.end()) {
    *out = it->second;
  } else {
    const double tc = now_ms();
    hipGraph_t graph = nullptr;
    hipError_t be = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    if (be != hipSuccess) rc = fail(e, VC_EHIP, "hipStreamBeginCapture failed: %s", hipGetErrorString(be));
    for (int i = 0; i < G && rc == VC_OK; ++i) rc = decode_step(e, sa, B, rps, grouped, s, sess);
    if (be == hipSuccess) {
      hipError_t ce = hipStreamEndCapture(s, &graph);
      if (rc == VC_OK && ce != hipSuccess) rc = fail(e, VC_EHIP, "hipStreamEndCapture failed: %s", hipGetErrorString(ce));
    }
    e->host_ms[HM_CAPTURE] += now_ms() - tc;
    if (rc == VC_OK) {
      const double ti = now_ms();
      hipError_t ie = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
      if (ie != hipSuccess) rc = fail(e, VC_EHIP, "hipGraphInstantiate failed: %s", hipGetErrorString(ie));
      else e->graphs[key] = *out;
      e->host_ms[HM_INSTANTIATE] += now_ms() - ti;
    }
    if (graph) (void)hipGraphDestroy(graph);
  }
  return rc;
}
// every graph this call can need, captured before the caller starts its decode timer
int DecodeLoop::precapture() {
  e->host_ms[HM_CAPTURE] = e->host_ms[HM_INSTANTIATE] = 0;
  if (!sc.use_graph) return VC_OK;
  hipGraphExec_t exec = nullptr;
  int rc0 = exec_for(&exec);
  if (can_shrink)            // ... and the narrower widths a shrinking batch passes through
    for (int w = width_for(B0) / 2; w >= 1 && rc0 == VC_OK; w /= 2) {
      if (w >= B0) continue;
      B = w; sa = make_sample_args(e, w, rps);
      rc0 = exec_for(&exec);
    }
  return rc0;
}
int DecodeLoop::begin() {
  t1 = now_ms();
  HIPCHK(e, hipMemsetAsync(e->step_ctr, 0, sizeof(int), s));      // the loop's first step is step 0 of batch 0 (SampleArgs.host_live slots)
  e->repack_at.clear();
  over = launched >= max_steps;
  return VC_OK;
}
// One batch of G steps of the width in force - its captured graph, or G eager steps - and the pacing event `slot` behind it.  The only
// place a batch is launched: advance() below and a decode session's turn (vc_session_advance), which keeps its own batch count.
int DecodeLoop::queue_batch(int slot) {
  int rc = VC_OK;
  if (sc.use_graph) {
    hipGraphExec_t exec = nullptr;
    if ((rc = exec_for(&exec))) return rc;
    hipError_t le = hipGraphLaunch(exec, s);
    if (le != hipSuccess) return fail(e, VC_EHIP, "hipGraphLaunch failed: %s", hipGetErrorString(le));
  } else {
    for (int i = 0; i < G && rc == VC_OK; ++i) rc = decode_step(e, sa, B, rps, grouped, s, sess);
    if (rc) return rc;
  }
  hipError_t re = hipEventRecord(e->ev_pace[slot], s);
  if (re != hipSuccess) return fail(e, VC_EHIP, "hipEventRecord: %s", hipGetErrorString(re));
  return VC_OK;
}
// One turn: wait for the older of the two batches in flight, then queue the next one.  Sets `over` instead when the loop has ended.
int DecodeLoop::advance() {
  volatile int* live = e->h_flag + HF_ACTIVE;
  volatile int* live_n = e->h_flag + HF_LIVE0;                   // two slots: sequences still live as the LAST step of a batch of G steps found them
  if (over) return VC_OK;
  if (batch >= 2) {   // pace: at most two batches in flight; the older one must have ended before a third is queued
    hipError_t we = hipEventSynchronize(e->ev_pace[batch & 1]);
    if (we != hipSuccess) { over = true; return fail(e, VC_EHIP, "pacing event: %s", hipGetErrorString(we)); }
    complete = (batch - 1) * G;
    if (*live <= 0) { over = true; return VC_OK; }
    if (can_shrink) {
      // the slot of the batch whose end has just been waited for (launched two iterations ago): the batch still in flight writes
      // the other one, so the width schedule is the same in every run of the same call - and with it, in bf16, every sampled token
      const int n_live = live_n[batch & 1];
      const int w = n_live >= 1 ? width_for(n_live) : B;
      if (w < B) {
        RepackArgs ra;
        memset(&ra, 0, sizeof ra);
        ra.st = e->st; ra.st_fin = e->st_fin; ra.dec_h = e->dec_h; ra.row_seq = e->dec_row_seq; ra.row_pos = e->dec_row_pos;
        ra.logit_row = e->logit_row; ra.err = e->err_flag; ra.B_old = B; ra.B_new = w; ra.d = e->d;
        hipError_t re = vc_launch_repack(ra, s);
        if (re != hipSuccess) { over = true; return fail(e, VC_EHIP, "re-pack launch: %s", hipGetErrorString(re)); }
        B = w; sa = make_sample_args(e, w, rps);
        e->repack_at.push_back(batch);                  // counted in host_ms[HM_REPACKS] once the call knows its live steps (tts_run)
      }
    }
  }
  if (const int rc = queue_batch(batch & 1)) { over = true; return rc; }
  launched += G;
  ++batch;
  if (launched >= max_steps) over = true;
  return VC_OK;
}
void DecodeLoop::finish(int* steps_run) {
  e->host_ms[HM_LOOP] = now_ms() - t1;
  e->host_ms[HM_SPARE] = 0;
  e->host_ms[HM_LAUNCHED] = launched;                               // decode steps LAUNCHED (a multiple of steps_per_graph; the tail are no-ops)
  e->cur_rows = B;
  if (steps_run) *steps_run = launched;
}
}  // namespace vch
namespace {

int decode_loop(vc_engine* e, const SampleArgs& sa0, int B0, int rps, int groups, const vc_sample_cfg* sc, int max_steps, hipStream_t s) {
  DecodeLoop L;
  L.init(e, sa0, B0, rps, groups, sc, max_steps, s);
  int rc = L.begin();
  if (rc) return rc;
  while (rc == VC_OK && !L.over) rc = L.advance();
  L.finish(nullptr);
  return rc;
}

SeqState init_state(vc_engine* e, int Lx, int n_cols, bool tts, int n_spans) {
  SeqState st;
  memset(&st, 0, sizeof st);
  st.Lx = Lx; st.y_len = n_cols; st.prev_token = -1; st.n_spans = n_spans; st.kept = 1; st.group = -1;
  const vc_model_cfg& c = e->cfg;
  if (tts) {
    st.cap_len = Lx * (c.encodec_sr / 5);                 // voicecraft.py:1042
    st.min_gen = c.encodec_sr / 5;                        // :1024
    st.term_token = c.eos > 0 ? c.eos : c.eog;            // :938
    st.kill_token = c.eos > 0 ? c.eog : -1;               // :1091-1093
  } else {
    st.cap_len = Lx * 10;                                 // :751
    st.min_gen = -1;
    st.term_token = c.eog;
    st.kill_token = c.eos > 0 ? c.eos : -1;               // :816-818
  }
  return st;
}

int check_ready(vc_engine* e) {
  if (!e) return VC_EINVAL;
  if (!e->finalized) return fail(e, VC_ESTATE, "weights are not finalized (call vc_finalize_weights)");
  hipError_t err = hipSetDevice(e->device);
  if (err != hipSuccess) return fail(e, VC_EHIP, "hipSetDevice: %s", hipGetErrorString(err));
  return VC_OK;
}

}  // namespace
namespace vch __attribute__((visibility("hidden"))) {
// entry points that decode (or change what a decode step is): not while a streaming TTS call is open
int check_idle(vc_engine* e) {
  const int rc = check_ready(e);
  if (rc) return rc;
  if (e->ts) return fail(e, VC_ESTATE, "a streaming TTS call is open (vc_tts_stream_end closes it)");
  if (e->sess) return fail(e, VC_ESTATE, "a decode session is open (vc_session_close closes it)");
  return VC_OK;
}

int check_err_flag(vc_engine* e, hipStream_t s) {
  HIPCHK(e, hipMemcpyAsync(e->h_flag, e->err_flag, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
  if (const int bits = *e->h_flag) {
    (void)hipMemsetAsync(e->err_flag, 0, sizeof(int), s);   // already on the error path
    if (bits & 2)
      return fail(e, VC_EINVAL, "shared_text_prefix: a sequence's text differs from sequence 0's inside the shared prefix");
    if (bits & 4)
      return fail(e, VC_ESTATE, "internal: a re-pack found more live sequences than the narrower step has rows");
    if (bits & 8)
      return fail(e, VC_ESTATE, "internal: the samples of a best-of-N group were not on consecutive rows in sample order at their keep decision");
    return fail(e, VC_EINVAL, "token id out of range in x or y (text rows %d, audio vocab %d)", e->cfg.text_rows, e->V);
  }
  return VC_OK;
}
}  // namespace vch
namespace {

// ---- the checks of options that need a weight image or a request: they refuse before anything is set
int need_fr8(vc_engine* e, const char* name, int v0) {
  if (v0 <= 0 || e->has_fr8) return VC_OK;
  return fail(e, VC_ESTATE, "option '%s': this engine was created with VC_FINISHED_ROWS=0 and VC_FR_ONE=0 and holds no 8-channel weight images", name);
}
int need_qkv8(vc_engine* e, const char*, int v0) {
  if (!v0 || e->has_qkv8 || !vc_gemm_fr1_ok(3 * e->d, e->d, e->dtype, 4)) return VC_OK;
  return fail(e, VC_ESTATE, "option 'qkv_p8': this engine was created with VC_QKV_P8=0 or VC_FR_ONE=0 and holds no 8-channel image of the QKV matrix");
}
int need_qkv16(vc_engine* e, const char*, int v0) {
  if (!v0 || e->has_qkv16) return VC_OK;
  return fail(e, VC_ESTATE, "option 'qkv16': this engine holds no 16-channel image of the QKV matrix (packed for max_seqs > 16, or with VC_QKV16=1 at creation)");
}
// mask: 1 FFN-down, 4 QKV; a matrix without planes (fp32, narrow, refused, VC_W13=0) keeps its bf16 launch
int need_mask(vc_engine* e, const char* name, int v0) {
  return v0 < 0 || (v0 & ~5) ? fail(e, VC_EINVAL, "option '%s': %d is not a mask of 1 (FFN-down) and 4 (QKV)", name, v0) : VC_OK;
}
// the seven w8 options (W8_FORMS, vc_engine_host.h): on an engine that made the form's request, one of the form's values (where a
// matrix has both kinds of planes the w8 bit wins over the w13 bit)
int need_w8_form(vc_engine* e, const char* name, int v0) {
  for (const W8Form& f : W8_FORMS) {
    if (strcmp(name, f.option)) continue;
    if (!(e->*f.req)) return fail(e, VC_EINVAL, "option '%s': this engine was created without %s", f.option, f.request);
    return w8_value_ok(f, v0) ? VC_OK : fail(e, VC_EINVAL, "option '%s': %d is not %s", f.option, v0, f.value_text);
  }
  return fail(e, VC_EINVAL, "unknown option '%s'", name);
}
int need_kv8(vc_engine* e, const char*, int) {
  return e->kv8_req ? VC_OK : fail(e, VC_EINVAL, "option 'kv8': this engine was created without vc_request_kv8");
}

int nonzero(int v) { return v ? 1 : 0; }
int two_or_one(int v) { return v == 2 ? 2 : 1; }
int low6(int v) { return v & 63; }
int whole_tiles(int v) { return v / VC_ROWS * VC_ROWS; }

// Every option, once: vc_set_option, the VC_* presets at creation and the option text are all driven from this table (the fields' own
// comments in struct vc_engine say what each option does and why its default is what it is).  A value is "v0[,v1]": `pre` (if any), then
// the clamp to [lo, hi], give field f0; v1, where the option has a second field, is clamped the same way and optional.
// The option TEXT lists, in table order, the options that have a group tag - "tag=" in front of the first of a run with the same tag, a
// comma between its members, '|' between runs -, and keys the captured decode graphs: an option that shapes a decode step carries a tag.
struct Val { int vc_engine::*f; int lo, hi; };
struct OptDesc {
  const char *name, *env, *tag;
  Val v0;
  int (*pre)(int);
  Val v1;                                           // .f null: one value
  int (*check)(vc_engine*, const char* name, int v0);
  int vc_engine::*only_if;                          // in the text only on an engine where this field is set (null: always)
};
using E = vc_engine;
const OptDesc OPTIONS[] = {
    {"graph_steps", "VC_GRAPH_STEPS", "g", {&E::steps_per_graph, 1, 64}},
    // "mask[,kv]": the weight matrices streamed with the hint, and the decode attention's K/V loads (0 never, 1 always, 2 from two rows up)
    {"nt", "VC_NT", "nt", {&E::nt_decode, 0, 63}, low6, {&E::attn_nt, 0, 2}},
    {"finished_rows", "VC_FINISHED_ROWS", "fr", {&E::fr_rows, 0, VC_ROWS}, nullptr, {}, need_fr8},
    {"fr_pair", "VC_FR_PAIR", "fr", {&E::fr_pair, 0, 1}, nonzero},
    {"att_p16", "VC_ATT_P16", "fr", {&E::att_p16, 0, 1}, nonzero},
    {"hq", "VC_HQ", "fr", {&E::hq, 0, 1}, nonzero},
    {"tile_attn", "VC_TILE_ATTN", "ta", {&E::tile_attn, 1, 2}, two_or_one, {&E::tile_attn_min_rows, 64, INT_MAX}},
    {"fr_one", "VC_FR_ONE", "r1", {&E::fr_one, 0, 2}, nullptr, {}, need_fr8},
    {"attn_fast", "VC_ATTN_FAST", "r1", {&E::attn_fast, 0, 1}, nonzero},
    {"qkv_p8", "VC_QKV_P8", "r1", {&E::qkv_p8, 0, 2}, nullptr, {}, need_qkv8},      // 2: steps of 2..8 finished rows as well (rows_gemm_qp_k)
    {"qkv16", "VC_QKV16", "q16", {&E::qkv16, 0, 1}, nonzero, {}, need_qkv16},
    {"wide_heads", "VC_WIDE_HEADS", "q16", {&E::wide_heads, 0, 1}, nonzero},
    {"wide_gemm", "VC_WIDE_GEMM", "q16", {&E::wide_gemm, 0, 1}, nonzero},
    {"wd_stage", "VC_WD_STAGE", "q16", {&E::wd_stage, 0, 1}, nonzero},
    {"shrink", "VC_SHRINK", "sh", {&E::shrink, 0, 1}, nonzero},
    {"w13", "VC_W13", "w13", {&E::w13, 0, 5}, nullptr, {}, need_mask},
    {"w8", nullptr, "w8", {&E::w8, 0, 5}, nullptr, {}, need_w8_form, &E::w8_req},      // only an engine that requested the form has the option
    {"w8r", nullptr, "w8r", {&E::w8r, 0, 5}, nullptr, {}, need_w8_form, &E::w8r_req},   // likewise (vc_request_w8_rows)
    {"w8m", nullptr, "w8m", {&E::w8m, 0, 9}, nullptr, {}, need_w8_form, &E::w8m_req},   // likewise (vc_request_w8_mid)
    {"w8w", nullptr, "w8w", {&E::w8w, 0, 13}, nullptr, {}, need_w8_form, &E::w8w_req},  // likewise (vc_request_w8_wide)
    {"w8u", nullptr, "w8u", {&E::w8u, 0, 10}, nullptr, {}, need_w8_form, &E::w8u_req},  // likewise (vc_request_w8_up)
    {"w8ur", nullptr, "w8ur", {&E::w8ur, 0, 10}, nullptr, {}, need_w8_form, &E::w8ur_req},   // likewise (vc_request_w8_up_rows)
    {"w8q", nullptr, "w8q", {&E::w8q, 0, 12}, nullptr, {}, need_w8_form, &E::w8q_req},   // likewise (vc_request_w8_qkv_rows)
    {"kv8", nullptr, "kv8", {&E::kv8, 0, 1}, nonzero, {}, need_kv8, &E::kv8_req},   // likewise
    {"prefill_rows", "VC_PREFILL_ROWS", nullptr, {&E::prefill_rows_per_pass, VC_ROWS, VC_MAX_ROWS}, whole_tiles},   // 16: decode kernels only
};

// One option by name (vc_set_option, and the VC_* environment variables at creation).
int apply_option(vc_engine* e, const std::string& name, const char* value) {
  int v[3] = {0, 0, 0};
  const int n = sscanf(value ? value : "", "%d,%d,%d", &v[0], &v[1], &v[2]);
  if (n < 1) return fail(e, VC_EINVAL, "option '%s': '%s' is not a number list", name.c_str(), value ? value : "(null)");
  for (const OptDesc& o : OPTIONS) {
    if (name != o.name) continue;
    if (o.check)
      if (const int rc = o.check(e, o.name, v[0])) return rc;
    e->*o.v0.f = std::max(o.v0.lo, std::min(o.pre ? o.pre(v[0]) : v[0], o.v0.hi));
    if (o.v1.f && n >= 2) e->*o.v1.f = std::max(o.v1.lo, std::min(v[1], o.v1.hi));
    return VC_OK;
  }
  return fail(e, VC_EINVAL, "unknown option '%s'", name.c_str());
}

void refresh_opt_state(vc_engine* e) {
  std::string& t = e->opt_state;
  t.clear();
  const char* tag = "";
  for (const OptDesc& o : OPTIONS) {
    if (!o.tag || (o.only_if && !(e->*o.only_if))) continue;
    if (strcmp(tag, o.tag)) t += std::string(t.empty() ? "" : "|") + o.tag + "=";
    else t += ",";
    tag = o.tag;
    t += std::to_string(e->*o.v0.f);
    if (o.v1.f) t += "," + std::to_string(e->*o.v1.f);
  }
  if (e->kv8c_req) t += "|kv8c=1";      // no option: an engine with vc_request_kv8c says so (the decode graphs are keyed by "kv8" in front of it)
}

int apply_env_presets(vc_engine* e) {
  for (const OptDesc& o : OPTIONS)
    if (const char* v = o.env ? getenv(o.env) : nullptr) {
      // (VC_NT was a boolean through round 3 - 1 = on, the default; it is a per-matrix bit mask now: the legacy "1" keeps meaning "on")
      if (!strcmp(o.env, "VC_NT") && !strcmp(v, "1")) v = "63";
      if (const int rc = apply_option(e, o.name, v)) return rc;
    }
  refresh_opt_state(e);
  return VC_OK;
}

// The stand-in engine of the host-only plans (vc_debug_plan, vc_debug_w8*_plan): this model shape and compute dtype, default options,
// the weight images vc_finalize_weights packs for an engine that takes wide steps.  VC_EINVAL for arguments no such engine has.
int plan_engine(vc_engine& e, const vc_model_cfg* c, int dtype, int rows, const void* out) {
  if (!c || !out || rows < 1 || rows > VC_MAX_SEQS || c->d_model <= 0 || c->nhead <= 0 || c->d_model % c->nhead) return VC_EINVAL;
  e.cfg = *c; e.d = c->d_model; e.H = c->nhead; e.hd = c->d_model / c->nhead; e.P = c->head_hidden; e.dtype = dtype;
  e.has_fr8 = e.has_qkv16 = true;
  e.has_qkv8 = vc_gemm_fr1_ok(3 * e.d, e.d, dtype, 4) != 0;
  return VC_OK;
}
// ... in bf16 with vc_request_w8(5) and the form's own request made, every matrix taken as packed, and the form's option = mask
int plan_engine_w8(vc_engine& e, const vc_model_cfg* c, int form, int mask, int rows, const void* out) {
  const W8Form& f = W8_FORMS[form];
  if (!w8_value_ok(f, mask)) return VC_EINVAL;
  if (const int rc = plan_engine(e, c, VC_DTYPE_BF16, rows, out)) return rc;
  e.w8_req = e.w8 = 5;
  e.*f.req = f.bits; e.*f.value = mask;
  return VC_OK;
}

// vc_request_w8*: every request comes before vc_finalize_weights; the masks of a form and their order after vc_request_w8 are the
// table's (W8Form, vc_engine_host.h).  The option starts at the mask that was asked for.
int request_w8_form(vc_engine* e, int form, int mask) {
  const W8Form& f = W8_FORMS[form];
  if (!e) return VC_EINVAL;
  if (e->finalized) return fail(e, VC_ESTATE, "%s comes before vc_finalize_weights", f.request);
  const bool after_w8 = form != W8F_ONE;
  if (f.subset) {
    if (mask < 0 || (mask & ~5)) return fail(e, VC_EINVAL, "%s: %d is not %s", f.request, mask, f.mask_text);
    if (after_w8 && !e->w8_req) return fail(e, VC_ESTATE, "%s comes after vc_request_w8", f.request);
    if (after_w8 && (mask & ~e->w8_req)) return fail(e, VC_EINVAL, "%s: mask %d is no subset of vc_request_w8's %d", f.request, mask, e->w8_req);
    if (mask & ~f.bits) return fail(e, VC_EINVAL, "%s: %s", f.request, f.no_form);
  } else {
    if (!e->w8_req) return fail(e, VC_ESTATE, "%s comes after vc_request_w8", f.request);
    if (mask != f.bits) return fail(e, VC_EINVAL, "%s: %d is not %s", f.request, mask, f.mask_text);
  }
  e->*f.req = mask;
  e->*f.value = mask;
  return VC_OK;
}

}  // namespace

// =====================================================================================  C ABI
// Host-only: what the kv8 options add to a pass (kv8_plan above, the function site_attn and run_pass follow).
extern "C" int vc_debug_kv8_plan(int request, int kv8, int rps, int rows_attn, int32_t out[4]) {
  if (!out || request < 0 || request > 2 || rps < 0) return VC_EINVAL;
  const Kv8Plan k = kv8_plan(request, kv8, rps, rows_attn != 0);
  out[0] = k.attn; out[1] = k.n_tail; out[2] = k.n_tail > 0 ? k.tail[0] : 0; out[3] = k.n_tail > 1 ? k.tail[1] : 0;
  return VC_OK;
}
// Host-only: what option "w8r" = mask makes of a bf16 decode pass of `rows` rows at this model shape, every matrix taken as packed
// (plan_pass itself, the function the sites follow).
extern "C" int vc_debug_w8r_plan(const vc_model_cfg* c, int mask, int rows, int32_t out[4]) {
  vc_engine e;
  if (const int rc = plan_engine_w8(e, c, W8F_ROWS, mask, rows, out)) return rc;
  const int d = e.d;
  const PassPlan p = plan_pass(&e, rows, true, 0);
  out[0] = p.frp_w8 ? 1 : 0;
  out[1] = p.qp_w8 ? 1 : 0;
  out[2] = p.frp_w8 ? vc_packed(VC_PK_W8).frp_ng(rows, d, 4 * d, e.dtype) : 0;
  out[3] = p.qp_w8 ? vc_packed(VC_PK_W8).qp_ng(rows, 3 * d, d, e.dtype) : 0;
  return VC_OK;
}
// Host-only: what option "w8m" = mask (bits 1, 8) makes of a bf16 decode pass of `rows` rows at this model shape, the matrix taken as
// packed (plan_pass itself): out = {form taken, kernel (1 = X in one piece, 2 = K in two halves), groups per wave and piece, 0}.
extern "C" int vc_debug_w8m_plan(const vc_model_cfg* c, int mask, int rows, int32_t out[4]) {
  vc_engine e;
  if (const int rc = plan_engine_w8(e, c, W8F_MID, mask, rows, out)) return rc;
  const int d = e.d;
  const PassPlan p = plan_pass(&e, rows, true, 0);
  out[0] = p.fr_w8_f2 ? 1 : 0;
  out[1] = p.fr_w8_f2 ? vc_gemm_fr_form(rows, d, 4 * d, e.dtype, PRO_PLAIN, 1) : 0;
  out[2] = p.fr_w8_f2 ? vc_packed(VC_PK_W8).fr_ng(rows, d, 4 * d, e.dtype) : 0;
  out[3] = 0;
  return VC_OK;
}
// Host-only: what option "w8w" = mask (bits 1, 4, 8) makes of a bf16 decode pass of `rows` rows at this model shape, every matrix taken
// as packed (plan_pass itself): out = {FFN-down on the pair planes, QKV on them, k-tiles per wave of the FFN-down slice, of the QKV matrix}.
extern "C" int vc_debug_w8w_plan(const vc_model_cfg* c, int mask, int rows, int32_t out[4]) {
  vc_engine e;
  if (const int rc = plan_engine_w8(e, c, W8F_WIDE, mask, rows, out)) return rc;
  const int d = e.d;
  const PassPlan p = plan_pass(&e, rows, true, 0);
  out[0] = p.wd_w8_f2 ? 1 : 0;
  out[1] = p.wd_w8_qkv ? 1 : 0;
  out[2] = p.wd_w8_f2 ? vc_gemm_wd_kpw(4 * d, e.dtype, p.ks_f2) : 0;
  out[3] = p.wd_w8_qkv ? vc_gemm_wd_kpw(d, e.dtype, 1) : 0;
  return VC_OK;
}
// Host-only: what option "w8u" = mask (0, 2 or 10) makes of a bf16 decode pass of `rows` rows at this model shape, W1 taken as packed
// (plan_pass itself): out = {FFN-up on the pair planes, k-tiles per wave there}.
extern "C" int vc_debug_w8u_plan(const vc_model_cfg* c, int mask, int rows, int32_t out[2]) {
  vc_engine e;
  if (const int rc = plan_engine_w8(e, c, W8F_UP, mask, rows, out)) return rc;
  const int d = e.d;
  const PassPlan p = plan_pass(&e, rows, true, 0);
  out[0] = p.wd_w8_f1 ? 1 : 0;
  out[1] = p.wd_w8_f1 ? vc_gemm_wd_kpw(d, e.dtype, 1) : 0;
  return VC_OK;
}
// Host-only: what option "w8ur" = mask (0, 2 or 10) makes of a bf16 decode pass of `rows` rows at this model shape, W1 taken as packed
// (plan_pass itself): out = {FFN-up of the finished rows on the pair planes, k-tiles per wave there}.
extern "C" int vc_debug_w8ur_plan(const vc_model_cfg* c, int mask, int rows, int32_t out[2]) {
  vc_engine e;
  if (const int rc = plan_engine_w8(e, c, W8F_UP_ROWS, mask, rows, out)) return rc;
  const int d = e.d;
  const PassPlan p = plan_pass(&e, rows, true, 0);
  out[0] = p.lnq_w8_f1 ? 1 : 0;
  out[1] = p.lnq_w8_f1 ? vc_packed(VC_PK_W8).lnq_ok(rows, 4 * d, d, e.dtype) : 0;
  return VC_OK;
}
// Host-only: what option "w8q" = mask (0, 4 or 12) makes of a bf16 decode pass of `rows` rows at this model shape, Wqkv taken as packed
// (plan_pass itself): out = {QKV of the finished rows of layers 1.. on the pairs of the 12-channel image, k-tiles per wave there}.
extern "C" int vc_debug_w8q_plan(const vc_model_cfg* c, int mask, int rows, int32_t out[2]) {
  vc_engine e;
  if (const int rc = plan_engine_w8(e, c, W8F_QKV_ROWS, mask, rows, out)) return rc;
  const int d = e.d;
  const PassPlan p = plan_pass(&e, rows, true, 0);
  out[0] = p.qkvq_w8 ? 1 : 0;
  out[1] = p.qkvq_w8 ? vc_packed(VC_PK_W8).qkvq_ok(rows, 3 * d, d, e.dtype) : 0;
  return VC_OK;
}
// Host-only: how a decode pass of `rows` rows would be launched for this model shape and compute dtype (no engine, no GPU).
extern "C" int vc_debug_plan(const vc_model_cfg* c, int compute_dtype, int rows, int32_t out[16]) {
  if (compute_dtype != VC_DTYPE_BF16 && compute_dtype != VC_DTYPE_F32) return VC_EINVAL;
  vc_engine e;
  if (const int rc = plan_engine(e, c, compute_dtype, rows, out)) return rc;
  const int d = e.d;
  const PassPlan p = plan_pass(&e, rows, true, 0);
  const bool fr = p.form == FORM_FR;
  out[0] = fr_max_rows(&e);
  out[1] = p.form;                                                            // 0 slab form (rows-GEMM), 1 finished-row form, 2 wide decode
  out[2] = p.nsplit;                                                          // attention splits
  out[3] = fr ? p.mt : -1;                                                    // consumers: GemmArgs.mt (0 one tile, 3 two tiles, 4 two tiles x two rows per wave)
  out[4] = fr ? vc_gemm_fr_form(rows, d, d, compute_dtype, p.att_x ? PRO_PLAIN : PRO_ATT, p.nsplit) : -1;   // out-projection producer form
  out[5] = fr ? vc_gemm_fr_form(rows, d, 4 * d, compute_dtype, PRO_PLAIN, 1) : -1;                       // FFN-down producer form
  out[6] = p.heads_fold ? 1 : 0;                                              // heads-1 folds finished rows itself (else LayerNorm launch)
  out[7] = (3 * d / VC_TH_QKV) % 2 == 0 && (4 * d / 16) % 2 == 0 ? 1 : 0;     // the consumers' tile counts are even (two tiles per workgroup)
  // the default forms of rounds 5-6
  for (int i = 8; i < 16; ++i) out[i] = -1;
  if (rows == 1) {
    out[8] = p.fd ? 1 : 0;                                                    // fr_one: FFN-down finishes its row
    out[9] = p.qkv_fr1 ? 1 : 0;                                               // qkv_p8: the paired QKV projection behind it
  }
  if (fr && rows <= VC_FR_MAX_ROWS) {
    out[10] = p.frp ? 1 : 0;                                                  // fr_pair
    out[9] = p.qp ? 2 : 0;                                                    // qkv_p8 = 2: layers 1.. run the QKV projection on rows_gemm_qp_k
  }
  if (rows > VC_ROWS) {
    out[11] = p.wd ? 1 : 0;                                                   // the wide step on rows_gemm_wd_k, and the launcher's forms it needs:
    out[12] = wd_ksplit(&e, d, d); out[13] = wd_ksplit(&e, d, 4 * d);
    out[14] = vc_gemm_wd_kpw(d, compute_dtype, 1); out[15] = vc_gemm_wd_kpw(c->head_hidden, compute_dtype, 1);
  }
  return VC_OK;
}

extern "C" int vc_set_option(vc_engine* e, const char* name, const char* value) {
  int rc = check_idle(e);
  if (rc) return rc;
  if (!name || !value) return fail(e, VC_EINVAL, "null argument to vc_set_option");
  rc = apply_option(e, name, value);
  refresh_opt_state(e);
  return rc;
}

extern "C" const char* vc_version(void) { return "vcengine 0.1 (gfx950)"; }

extern "C" const char* vc_last_error(const vc_engine* e) { return e ? e->err.c_str() : g_create_err.c_str(); }

extern "C" int vc_create(const vc_model_cfg* c, int hip_device, vc_engine** out) {
  if (!c || !out) return fail(nullptr, VC_EINVAL, "null argument");
  *out = nullptr;
  if (c->d_model <= 0 || c->d_model % 256 || c->d_model > 2048)
    return fail(nullptr, VC_EINVAL, "d_model %d must be a multiple of 256 and <= 2048", c->d_model);
  if (c->nhead <= 0 || c->d_model % c->nhead) return fail(nullptr, VC_EINVAL, "nhead %d does not divide d_model", c->nhead);
  const int hd = c->d_model / c->nhead;
  if (hd != 32 && hd != 64 && hd != 128)   // the attention kernel spreads a cached row over 4, 8, 16 or 32 lanes
    return fail(nullptr, VC_EINVAL, "head_dim %d must be 32, 64 or 128", hd);
  if ((hd & (hd - 1)) != 0) return fail(nullptr, VC_EINVAL, "head_dim %d must be a power of two", hd);
  if (c->n_codebooks < 2)   // voicecraft.py:967, :1217 cut the shifted prompt with [:, :-(n_codebooks-1)]: at K = 1 that is [:, :-0], nothing is left
    return fail(nullptr, VC_EINVAL, "n_codebooks %d unsupported: the reference's own TTS drops the whole audio prompt at one codebook "
                "([:, :-(n_codebooks-1)]), so there is nothing to be equal to; 2..%d are supported", c->n_codebooks, VC_MAX_CODEBOOKS);
  if (c->n_codebooks > VC_MAX_CODEBOOKS) return fail(nullptr, VC_EINVAL, "n_codebooks %d unsupported (max %d)", c->n_codebooks, VC_MAX_CODEBOOKS);
  const int V = c->audio_vocab_size + c->n_special;
  if (V > 64 * VC_VPL) return fail(nullptr, VC_EINVAL, "audio vocabulary %d too large (max %d)", V, 64 * VC_VPL);
  if (c->head_hidden % 256) return fail(nullptr, VC_EINVAL, "head_hidden %d must be a multiple of 256", c->head_hidden);
  if (c->empty_token != c->audio_vocab_size || c->eog != c->audio_vocab_size + 1 ||
      c->audio_pad_token != c->audio_vocab_size + 2)   // voicecraft.py:132-134
    return fail(nullptr, VC_EINVAL, "special tokens must be empty=V, eog=V+1, pad=V+2");
  if (c->eos >= V || c->eog >= V) return fail(nullptr, VC_EINVAL, "eos/eog outside the vocabulary");
  if (c->max_seqs < 1 || c->max_seqs > VC_MAX_SEQS) return fail(nullptr, VC_EINVAL, "max_seqs must be in [1,%d]", VC_MAX_SEQS);
  if (c->max_positions < 32) return fail(nullptr, VC_EINVAL, "max_positions too small");
  if (c->max_n_spans < 1 || c->max_n_spans > VC_MAX_SPANS) return fail(nullptr, VC_EINVAL, "max_n_spans unsupported");
  hipError_t err = hipSetDevice(hip_device);
  if (err != hipSuccess) return fail(nullptr, VC_EHIP, "hipSetDevice(%d): %s", hip_device, hipGetErrorString(err));
  vc_engine* e = new vc_engine();
  e->cfg = *c; e->device = hip_device;
  e->d = c->d_model; e->H = c->nhead; e->hd = hd; e->L = c->num_layers; e->K = c->n_codebooks;
  e->V = V; e->P = c->head_hidden; e->S_max = c->max_positions; e->B_max = c->max_seqs;
  e->NS = std::max(VC_ROWS, c->max_seqs);
  *out = e;
  return VC_OK;
}

extern "C" void vc_destroy(vc_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  (void)hipDeviceSynchronize();
  for (auto& kv : e->raw) if (kv.second.dev) (void)hipFree(kv.second.dev);
  for (void* p : e->allocs) (void)hipFree(p);
  if (e->eval_logits) (void)hipFree(e->eval_logits);
  if (e->h_st) (void)hipHostFree(e->h_st);
  if (e->h_st2) (void)hipHostFree(e->h_st2);
  if (e->h_flag) (void)hipHostFree(e->h_flag);
  if (e->h_dyn) (void)hipHostFree(e->h_dyn);
  for (auto& kv : e->graphs) if (kv.second) (void)hipGraphExecDestroy(kv.second);
  for (auto& ev : e->ev_pace) if (ev) (void)hipEventDestroy(ev);
  for (auto& ev : e->ev) if (ev) (void)hipEventDestroy(ev);
  if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
  if (e->side_stream) (void)hipStreamDestroy(e->side_stream);
  drop_tts_stream(e);
  drop_session(e);
  if (e->h_rec) (void)hipHostFree(e->h_rec);
  if (e->h_adm_st) (void)hipHostFree(e->h_adm_st);
  if (e->h_adm_ctl) (void)hipHostFree(e->h_adm_ctl);
  delete e;
}

extern "C" int vc_load_tensor(vc_engine* e, const char* key, const void* data, int on_device, int dtype,
                              const int64_t* shape, int ndim) {
  if (!e || !key || !data || ndim < 0 || ndim > 4) return fail(e, VC_EINVAL, "bad argument to vc_load_tensor");
  if (e->finalized) return fail(e, VC_ESTATE, "weights already finalized");
  if (dtype != VC_DTYPE_F32) return VC_OK;   // eog / eos buffers (int64) carry no information we need
  HIPCHK(e, hipSetDevice(e->device));
  RawTensor t;
  t.numel = 1;
  for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); t.numel *= shape[i]; }
  if (t.numel <= 0) return fail(e, VC_EINVAL, "empty tensor '%s'", key);
  auto it = e->raw.find(key);
  if (it != e->raw.end()) { (void)hipFree(it->second.dev); e->raw.erase(it); }
  HIPCHK(e, hipMalloc((void**)&t.dev, (size_t)t.numel * 4));
  HIPCHK(e, hipMemcpy(t.dev, data, (size_t)t.numel * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  e->raw[key] = t;
  return VC_OK;
}

// Asks vc_finalize_weights to pack the matrices of `mask` (1 FFN-down, 4 QKV) as E4M3 bytes too (option "w8").  The compute dtype is
// chosen at vc_finalize_weights, so that is where a request meets an fp32 engine: VC_EINVAL from there.
extern "C" int vc_request_w8(vc_engine* e, int mask) { return request_w8_form(e, W8F_ONE, mask); }

// Lets steps of 2..8 finished rows stream the planes vc_request_w8 asked for (option "w8r"): `mask` is a subset of that request's.
extern "C" int vc_request_w8_rows(vc_engine* e, int mask) { return request_w8_form(e, W8F_ROWS, mask); }

// Lets steps of 17..64 rows stream the matrices of `mask` (a subset of vc_request_w8's) as E4M3 pair planes of their 16-channel images
// (option "w8w"): packed at vc_finalize_weights, + 0.5 x the two images, on an engine that can run wide steps.
extern "C" int vc_request_w8_wide(vc_engine* e, int mask) { return request_w8_form(e, W8F_WIDE, mask); }

// Lets steps of 17..64 rows stream the FFN up-projection (mask 2, nothing else) as E4M3 pair planes of its 16-channel image W1 (option
// "w8u"): packed at vc_finalize_weights, + 0.5 x that image, on an engine that can run wide steps.  Needs vc_request_w8 (the bf16 /
// fp32 check of that request at vc_finalize_weights covers this one) but none of its bits, and not vc_request_w8_wide.
extern "C" int vc_request_w8_up(vc_engine* e, int mask) { return request_w8_form(e, W8F_UP, mask); }

// Lets passes of 2..16 finished rows stream the FFN up-projection (mask 2, nothing else) from the pair planes of W1 (option "w8ur"):
// the planes option "w8u" streams at 17..64 rows, packed at vc_finalize_weights whatever max_seqs is - once when both are requested.
// Needs vc_request_w8 (the bf16 / fp32 check of that request at vc_finalize_weights covers this one) but none of its bits.
extern "C" int vc_request_w8_up_rows(vc_engine* e, int mask) { return request_w8_form(e, W8F_UP_ROWS, mask); }

// Lets the finished-row passes whose QKV projection still reads the 12-channel image (9..16 rows; 7 and 8 at d = 2048) stream it (mask
// 4, nothing else) from the pairs of that image (option "w8q"): packed at vc_finalize_weights for layers 1.., + 0.5 x that image, whatever
// max_seqs is.  Needs vc_request_w8 (the bf16 / fp32 check of that request at vc_finalize_weights covers this one) but none of its bits.
extern "C" int vc_request_w8_qkv_rows(vc_engine* e, int mask) { return request_w8_form(e, W8F_QKV_ROWS, mask); }

// Lets passes of 9..16 finished rows stream the FFN-down planes vc_request_w8 asked for (option "w8m"): `mask` is bit 1 of that request.
// Nothing more is packed and resident memory does not change.
extern "C" int vc_request_w8_mid(vc_engine* e, int mask) { return request_w8_form(e, W8F_MID, mask); }

// Asks vc_finalize_weights for the E4M3 copy of the K / V cache (option "kv8").  As for vc_request_w8, an fp32 engine meets the request
// at vc_finalize_weights: VC_EINVAL from there.
extern "C" int vc_request_kv8(vc_engine* e) {
  if (!e) return VC_EINVAL;
  if (e->finalized) return fail(e, VC_ESTATE, "vc_request_kv8 comes before vc_finalize_weights");
  e->kv8_req = 1;
  e->kv8 = 1;
  return VC_OK;
}

// vc_request_kv8 with centred K (vc_kv8.h): the same rules, and implies it.
extern "C" int vc_request_kv8c(vc_engine* e) {
  if (!e) return VC_EINVAL;
  if (e->finalized) return fail(e, VC_ESTATE, "vc_request_kv8c comes before vc_finalize_weights");
  e->kv8_req = 1;
  e->kv8 = 1;
  e->kv8c_req = 1;
  return VC_OK;
}

namespace {

// dalloc, and the first `zero` bytes of the buffer cleared (the device words are four ints each: most are cleared as those 16 bytes)
template <typename T>
int dalloc0(vc_engine* e, T** p, size_t n, size_t zero) {
  if (const int rc = dalloc(e, p, n)) return rc;
  HIPCHK(e, hipMemset(*p, 0, zero));
  return VC_OK;
}

// The steps of vc_finalize_weights, in the order it calls them.  The order and the sizes of the allocations are behaviour: addresses
// in HBM follow from them, and the decode kernels' timings have been sensitive to placement.
// ---- embeddings (kept fp32: a handful of row gathers per step)
int load_embeddings(vc_engine* e) {
  const int d = e->d, K = e->K, V = e->V;
  int rc;
  const RawTensor* t;
  if ((rc = need(e, "text_embedding.word_embeddings.weight", {e->cfg.text_rows, d}, &t))) return rc;
  if ((rc = dalloc(e, &e->text_emb, (size_t)t->numel))) return rc;
  HIPCHK(e, hipMemcpy(e->text_emb, t->dev, (size_t)t->numel * 4, hipMemcpyDeviceToDevice));
  if ((rc = dalloc(e, &e->audio_emb, (size_t)K * V * d))) return rc;
  for (int k = 0; k < K; ++k) {
    if ((rc = need(e, "audio_embedding." + std::to_string(k) + ".word_embeddings.weight", {V, d}, &t))) return rc;
    HIPCHK(e, hipMemcpy(e->audio_emb + (size_t)k * V * d, t->dev, (size_t)V * d * 4, hipMemcpyDeviceToDevice));
  }
  if ((rc = need(e, "mask_embedding", {e->cfg.max_n_spans, d}, &t))) return rc;
  if ((rc = dalloc(e, &e->mask_emb, (size_t)t->numel))) return rc;
  HIPCHK(e, hipMemcpy(e->mask_emb, t->dev, (size_t)t->numel * 4, hipMemcpyDeviceToDevice));
  if ((rc = need(e, "text_positional_embedding.alpha", {1}, &t))) return rc;
  HIPCHK(e, hipMemcpy(&e->alpha_text, t->dev, 4, hipMemcpyDeviceToHost));
  if ((rc = need(e, "audio_positional_embedding.alpha", {1}, &t))) return rc;
  HIPCHK(e, hipMemcpy(&e->alpha_audio, t->dev, 4, hipMemcpyDeviceToHost));
  return VC_OK;
}

// ---- sinusoidal table (embedding.py:69-92).  "pe" may be supplied by the loader (torch's own
// sin/cos); otherwise it is computed here in fp32 with the same formula.
int load_position_table(vc_engine* e) {
  const int d = e->d;
  int rc;
  if ((rc = dalloc(e, &e->pe, (size_t)e->S_max * d))) return rc;
  if (const RawTensor* pt = find_raw(e, "pe")) {
    if (pt->shape.size() != 2 || pt->shape[0] < e->S_max || pt->shape[1] != d)
      return fail(e, VC_EINVAL, "'pe' must be [>=%d][%d]", e->S_max, d);
    HIPCHK(e, hipMemcpy(e->pe, pt->dev, (size_t)e->S_max * d * 4, hipMemcpyDeviceToDevice));
  } else {
    std::vector<float> pe((size_t)e->S_max * d);
    for (int i = 0; i < d; i += 2) {
      const float div = expf((float)i * -(logf(10000.0f) / (float)d));
      for (int p = 0; p < e->S_max; ++p) {
        const float a = (float)p * div;
        pe[(size_t)p * d + i] = sinf(a);
        pe[(size_t)p * d + i + 1] = cosf(a);
      }
    }
    HIPCHK(e, hipMemcpy(e->pe, pe.data(), pe.size() * 4, hipMemcpyHostToDevice));
  }
  return VC_OK;
}

// ---- which images and planes the decoder layers get: decided at creation, from the VC_* presets
void decide_images(vc_engine* e) {
  const int d = e->d;
  const char* env_fr = getenv("VC_FINISHED_ROWS");
  const char* env_f1 = getenv("VC_FR_ONE");
  const bool want_fr8 = !(env_fr && atoi(env_fr) == 0 && env_f1 && atoi(env_f1) == 0);
  // the 16-channel image of the QKV matrix serves wide decode steps (17..64 rows) and prefill passes: packed for engines that can
  // take such steps (max_seqs > 16) or on request (VC_QKV16=1); a narrower engine runs its prefill on the 12-channel tiles (-0.4 GB)
  const char* env_q16 = getenv("VC_QKV16");
  const bool want_qkv16 = env_q16 ? atoi(env_q16) != 0 : e->B_max > VC_ROWS;
  if (!want_qkv16) e->qkv16 = 0;
  const char* env_p8 = getenv("VC_QKV_P8");
  const bool want_p8 = !(env_p8 && atoi(env_p8) == 0) && !(env_f1 && atoi(env_f1) == 0);
  e->has_fr8 = want_fr8;
  e->has_qkv8 = want_fr8 && want_p8 && vc_gemm_fr1_ok(3 * d, d, e->dtype, 4);
  e->has_qkv16 = want_qkv16;
  const char* env_w13 = getenv("VC_W13");
  e->has_w13 = e->dtype == VC_DTYPE_BF16 && !(env_w13 && atoi(env_w13) == 0);
}

// ---- decoder layer l: its images, their 8- and 16-channel twins and packed planes, its K/V cache (and the kv8 copy); frees its staging
int pack_layer(vc_engine* e, int l) {
  const int d = e->d;
  const bool want_fr8 = e->has_fr8, want_qkv16 = e->has_qkv16;
  int rc;
  const std::string pre = "decoder.layers." + std::to_string(l) + ".";
  Layer& ly = e->layers[l];
  if ((rc = pack_folded(e, pre + "self_attn.in_proj_weight", pre + "self_attn.in_proj_bias", pre + "norm1.", 3 * d, d,
                        &ly.Wqkv, &ly.wg_qkv, &ly.bqkv, VC_TH_QKV))) return rc;
  if (want_qkv16) {
    const RawTensor* tg1;
    if ((rc = need(e, pre + "norm1.weight", {d}, &tg1))) return rc;
    if ((rc = pack_matrix(e, pre + "self_attn.in_proj_weight", 3 * d, d, &ly.Wqkv16, 16, tg1->dev))) return rc;
  }
  if ((rc = pack_matrix(e, pre + "self_attn.out_proj.weight", d, d, &ly.Wo))) return rc;
  if ((rc = keep_vec(e, pre + "self_attn.out_proj.bias", d, &ly.bo, &ly.bo_mean))) return rc;
  if ((rc = pack_folded(e, pre + "linear1.weight", pre + "linear1.bias", pre + "norm2.", 4 * d, d,
                        &ly.W1, &ly.wg_1, &ly.b1))) return rc;
  if ((rc = pack_matrix(e, pre + "linear2.weight", d, 4 * d, &ly.W2))) return rc;
  // the second, 8-channel-tile image of the two row-producing matrices (finished-row forms): + 10 d^2 elements per layer = + 0.67 GB
  // at giga830M in bf16.  An engine created with BOTH forms preset off (VC_FINISHED_ROWS=0 and VC_FR_ONE=0) does not pack them,
  // and refuses to switch the forms on later (apply_option).
  if (want_fr8) {
    if ((rc = pack_matrix(e, pre + "self_attn.out_proj.weight", d, d, &ly.Wo8, VC_TH_RES))) return rc;
    if ((rc = pack_matrix(e, pre + "linear2.weight", d, 4 * d, &ly.W28, VC_TH_RES))) return rc;
    // (the one-row paired QKV kernel reads the folded matrix in 8-channel tiles: only where its form can run, i.e. behind fr_one)
    // (not packed when either of the two options it serves is preset off - VC_QKV_P8=0 / VC_FR_ONE=0 -: 0.4 GB at giga830M)
    if (e->has_qkv8) {
      const RawTensor* tg1;
      if ((rc = need(e, pre + "norm1.weight", {d}, &tg1))) return rc;
      if ((rc = pack_matrix(e, pre + "self_attn.in_proj_weight", 3 * d, d, &ly.Wqkv8, VC_TH_RES, tg1->dev))) return rc;
    }
  }
  if ((rc = keep_vec(e, pre + "linear2.bias", d, &ly.b2, &ly.b2_mean))) return rc;
  // two of the big matrices of a one-row step once more as 13-bit planes, where a wave's share is whole groups of four fragments
  // (vc_gemm_packed_fr1_ng: FFN-down from d = 512, QKV from d = 1024), and, only for an engine that asked (vc_request_w8), the
  // requested ones as E4M3 bytes: the same widths, + 0.5 x the requested images
  // the group planes of `kind` (VC_PK_*) of an image of `n_frags` 1 KB fragments: one side byte per fragment
  auto pack_planes = [&](int kind, int which, const uint4* image, long n_frags) {
    const vc_packed_kind& pk = vc_packed(kind);
    return pack_checked(e, ly.packed[kind][which], (size_t)(n_frags / pk.group_frags) * pk.group_u4, (size_t)(n_frags / 4),
                        [&](uint4* planes, unsigned char* side, unsigned int* counts) { return pk.pack(image, n_frags, planes, side, counts, 0); });
  };
  // the pair planes (vc_w8.h "w8w", slot PK_W8W) of a 16-channel image of `n_pairs` pairs: two side bytes per pair
  auto pack_pairs = [&](int which, const uint4* image, long n_pairs) {
    return pack_checked(e, ly.packed[PK_W8W][which], (size_t)n_pairs * VC_W8W_PAIR_U4, (size_t)(n_pairs + 1) / 2,
                        [&](uint4* planes, unsigned char* side, unsigned int* counts) { return vc_launch_w8w_pack(image, n_pairs, planes, side, counts, 0); });
  };
  const int pack_mask[VC_PK_N] = {e->has_w13 ? 5 : 0, e->w8_req};
  for (int kind = 0; kind < VC_PK_N; ++kind) {
    if ((pack_mask[kind] & W8_BITS[W13_F2]) && ly.W28 && vc_gemm_packed_fr1_ng(kind, d, 4 * d, e->dtype, VC_FR_WAVES) &&
        (rc = pack_planes(kind, W13_F2, ly.W28, (long)(d / VC_TH_RES) * (4 * d / 64)))) return rc;
    if ((pack_mask[kind] & W8_BITS[W13_QKV]) && ly.Wqkv8 && vc_gemm_packed_fr1_ng(kind, 3 * d, d, e->dtype, 4) &&
        (rc = pack_planes(kind, W13_QKV, ly.Wqkv8, (long)(3 * d / VC_TH_RES) * (d / 64)))) return rc;
  }
  // on request (vc_request_w8_wide), for an engine that can run wide steps: the 16-channel images W2 / Wqkv16 as pair planes, where
  // the wide kernel has a form on them for the K slice it would use (+ 0.5 x the two images)
  if (e->w8w_req && want_qkv16 && e->dtype == VC_DTYPE_BF16) {
    const vc_packed_kind& pk8 = vc_packed(VC_PK_W8);
    if ((e->w8w_req & W8_BITS[W13_F2]) && pk8.wd_ok(4 * d, e->dtype, std::max(1, wd_ksplit(e, d, 4 * d))) &&
        (rc = pack_pairs(W13_F2, ly.W2, (long)(d / 16) * (4 * d / 64)))) return rc;
    if ((e->w8w_req & W8_BITS[W13_QKV]) && ly.Wqkv16 && pk8.wd_ok(d, e->dtype, 1) &&
        (rc = pack_pairs(W13_QKV, ly.Wqkv16, (long)(3 * d / 16) * (d / 64)))) return rc;
  }
  // on request (vc_request_w8_up), likewise: the 16-channel image W1 of the FFN up-projection (K = d in one slice): + 0.5 x the image
  // (vc_request_w8_up_rows: the same planes for passes of 2..16 finished rows, whatever max_seqs is - packed once when both ask)
  const bool up_wide = e->w8u_req && want_qkv16 && vc_packed(VC_PK_W8).wd_ok(d, e->dtype, 1);
  const bool up_rows = e->w8ur_req && vc_packed(VC_PK_W8).lnq_ok(2, 4 * d, d, e->dtype);
  if ((up_wide || up_rows) && e->dtype == VC_DTYPE_BF16 &&
      (rc = pack_pairs(W13_F1, ly.W1, (long)(4 * d / 16) * (d / 64)))) return rc;
  // on request (vc_request_w8_qkv_rows): the pairs of the 12-channel image Wqkv, for the layers that read a centred copy (layer 0 has
  // none and keeps PRO_LNW), whatever max_seqs is: + 0.5 x the image
  // (vc_w8.h "w8q", slot Layer::w8q: 768 B of codes and two side bytes per pair, d / 32 k-tiles per tile)
  const long pairs12 = (long)(3 * d / VC_TH_QKV) * (d / 64);
  if (e->w8q_req && l > 0 && e->dtype == VC_DTYPE_BF16 && vc_packed(VC_PK_W8).qkvq_ok(2, 3 * d, d, e->dtype) &&
      (rc = pack_checked(e, ly.w8q, (size_t)pairs12 * VC_W8Q_PAIR_U4, (size_t)(pairs12 + 1) / 2, [&](uint4* planes, unsigned char* side, unsigned int* counts) {
         return vc_launch_w8q_pack(ly.Wqkv, pairs12, d / 32, planes, side, counts, 0);
       }))) return rc;
  const size_t cache_bytes = (size_t)e->B_max * e->H * e->S_max * e->hd * e->esz;
  if ((rc = dalloc(e, &ly.kc, cache_bytes))) return rc;
  if ((rc = dalloc(e, &ly.vc, cache_bytes))) return rc;
  if (e->kv8_req) {
    const size_t vals = (size_t)e->B_max * e->H * e->S_max * e->hd;
    if ((rc = dalloc0(e, &ly.kc8, vals, vals)) || (rc = dalloc0(e, &ly.vc8, vals, vals)) ||
        (rc = dalloc0(e, &ly.sh8, vals / e->hd * 2, vals / e->hd * 2))) return rc;
  }
  // free the staging copies of this layer right away (3.3 GB for the 830M shape otherwise)
  for (const char* k2 : {"self_attn.in_proj_weight", "self_attn.out_proj.weight", "linear1.weight", "linear2.weight"}) {
    auto it = e->raw.find(pre + k2);
    if (it != e->raw.end()) { HIPCHK(e, hipDeviceSynchronize()); (void)hipFree(it->second.dev); e->raw.erase(it); }
  }
  return VC_OK;
}

// ---- option "kv8": the device table of the layers' five arrays
int upload_kv8_table(vc_engine* e) {
  int rc;
  std::vector<Kv8Layer> tab;
  for (const Layer& ly : e->layers) tab.push_back(Kv8Layer{ly.kc, ly.vc, ly.kc8, ly.vc8, ly.sh8});
  if ((rc = dalloc(e, &e->kv8_tab, tab.size()))) return rc;
  HIPCHK(e, hipMemcpy(e->kv8_tab, tab.data(), tab.size() * sizeof(Kv8Layer), hipMemcpyHostToDevice));
  if (!e->kv8c_req) return VC_OK;
  // centred K: the layers' centres (zero until a prefill pass leaves one), their table, n0 per slot - behind every allocation a plain
  // kv8 engine makes up to here
  const size_t cen_bytes = (size_t)e->B_max * e->H * e->hd * 2;
  std::vector<void*> cen;
  for (Layer& ly : e->layers) {
    if ((rc = dalloc(e, &ly.kcen, cen_bytes))) return rc;
    HIPCHK(e, hipMemset(ly.kcen, 0, cen_bytes));
    cen.push_back(ly.kcen);
  }
  if ((rc = dalloc(e, &e->kcen_tab, cen.size())) || (rc = dalloc0(e, &e->kcen_rows, (size_t)e->B_max, (size_t)e->B_max * sizeof(int)))) return rc;
  HIPCHK(e, hipMemcpy(e->kcen_tab, cen.data(), cen.size() * sizeof(void*), hipMemcpyHostToDevice));
  return VC_OK;
}

// ---- heads: first linears concatenated to one [K*P][d] matrix, second ones one group each
int pack_heads(vc_engine* e) {
  const int d = e->d, K = e->K, V = e->V, P = e->P;
  int rc;
  const RawTensor* t;
  // (folded with the final LayerNorm decoder.norm, transformer.py:484-485)
  float *cat, *bcat;
  const RawTensor *tg, *tbe;
  if ((rc = need(e, "decoder.norm.weight", {d}, &tg))) return rc;
  if ((rc = need(e, "decoder.norm.bias", {d}, &tbe))) return rc;
  HIPCHK(e, hipMalloc((void**)&cat, (size_t)K * P * d * 4));
  if (hipMalloc((void**)&bcat, (size_t)K * P * 4) != hipSuccess) { (void)hipFree(cat); return fail(e, VC_EHIP, "hipMalloc failed"); }
  auto drop = [&]() { (void)hipDeviceSynchronize(); (void)hipFree(cat); (void)hipFree(bcat); };
  if ((rc = dalloc(e, &e->bh1, (size_t)K * P))) { drop(); return rc; }
  if ((rc = dalloc(e, &e->wg_h1, (size_t)K * P))) { drop(); return rc; }
  for (int k = 0; k < K; ++k) {
    const std::string pre = "predict_layer." + std::to_string(k) + ".";
    if ((rc = need(e, pre + "0.weight", {P, d}, &t))) { drop(); return rc; }
    if (hipMemcpy(cat + (size_t)k * P * d, t->dev, (size_t)P * d * 4, hipMemcpyDeviceToDevice) != hipSuccess) { drop(); return fail(e, VC_EHIP, "hipMemcpy of %s0.weight failed", pre.c_str()); }
    if ((rc = need(e, pre + "0.bias", {P}, &t))) { drop(); return rc; }
    if (hipMemcpy(bcat + (size_t)k * P, t->dev, (size_t)P * 4, hipMemcpyDeviceToDevice) != hipSuccess) { drop(); return fail(e, VC_EHIP, "hipMemcpy of %s0.bias failed", pre.c_str()); }
  }
  const int KW = e->dtype == VC_DTYPE_BF16 ? 32 : 16;
  const long units = (long)(K * P / 16) * (d / KW) * 64;
  if ((rc = dalloc(e, &e->Wh1, (size_t)units))) { drop(); return rc; }
  hipError_t pe_ = vc_launch_pack(cat, tg->dev, e->Wh1, K * P, d, e->dtype, 16, 0);
  if (pe_ == hipSuccess) pe_ = vc_launch_fold_vecs(cat, tg->dev, tbe->dev, bcat, e->wg_h1, e->bh1, K * P, d, e->dtype, 0);
  drop();
  HIPCHK(e, pe_);
  const long gunits = (long)((V + 15) / 16) * (P / KW) * 64;
  e->wh2_group_stride = gunits;
  if ((rc = dalloc(e, &e->Wh2, (size_t)gunits * K))) return rc;
  if ((rc = dalloc(e, &e->bh2, (size_t)K * V))) return rc;
  for (int k = 0; k < K; ++k) {
    const std::string pre = "predict_layer." + std::to_string(k) + ".";
    if ((rc = need(e, pre + "2.weight", {V, P}, &t))) return rc;
    HIPCHK(e, vc_launch_pack(t->dev, nullptr, e->Wh2 + (size_t)k * gunits, V, P, e->dtype, 16, 0));
    if ((rc = need(e, pre + "2.bias", {V}, &t))) return rc;
    HIPCHK(e, hipMemcpy(e->bh2 + (size_t)k * V, t->dev, (size_t)V * 4, hipMemcpyDeviceToDevice));
  }
  return VC_OK;
}

// ---- launch plans
void make_plans(vc_engine* e) {
  const int d = e->d, K = e->K, V = e->V, P = e->P;
  e->p_qkv = make_plan(3 * d, d, e->dtype, false, nullptr, VC_TH_QKV);
  e->p_qkv16 = make_plan(3 * d, d, e->dtype, false, nullptr, 16);
  e->p_o = make_plan(d, d, e->dtype, true, "VC_KSPLIT_O");
  e->p_f1 = make_plan(4 * d, d, e->dtype, false, nullptr);
  e->p_f2 = make_plan(d, 4 * d, e->dtype, true, "VC_KSPLIT_F");
  e->p_h1 = make_plan(K * P, d, e->dtype, false, nullptr);
  e->p_h2 = make_plan(V, P, e->dtype, false, nullptr);
}

// ---- scratch arenas of a pass
int alloc_pass_arenas(vc_engine* e) {
  const int d = e->d, K = e->K, V = e->V, P = e->P;
  int rc;
  e->emb_cap = std::max(e->S_max, 8 * VC_MAX_ROWS);
  if ((rc = dalloc(e, &e->emb, (size_t)e->emb_cap * d))) return rc;
  if ((rc = dalloc(e, &e->pre_row_seq, (size_t)e->emb_cap + VC_MAX_ROWS))) return rc;
  if ((rc = dalloc(e, &e->pre_row_pos, (size_t)e->emb_cap + VC_MAX_ROWS))) return rc;
  if ((rc = dalloc(e, &e->hA, (size_t)VC_MAX_ROWS * d))) return rc;
  if ((rc = dalloc(e, &e->hB, (size_t)VC_MAX_ROWS * d))) return rc;
  if ((rc = dalloc(e, &e->q, (size_t)VC_MAX_ROWS * d))) return rc;
  if ((rc = dalloc(e, &e->parts, (size_t)VC_MAX_KSPLIT * VC_SLAB_ROWS * d))) return rc;
  if ((rc = dalloc(e, &e->att_o, (size_t)VC_ROWS * e->H * VC_MAX_NSPLIT * e->hd))) return rc;     // split partials: decode-size passes only
  if ((rc = dalloc(e, &e->att_ml, (size_t)VC_ROWS * e->H * VC_MAX_NSPLIT * 2))) return rc;
  if ((rc = dalloc(e, &e->act, (size_t)VC_MAX_ROWS * 4 * d * e->esz))) return rc;
  if ((rc = dalloc(e, &e->xn, (size_t)VC_MAX_ROWS * d * e->esz))) return rc;
  if ((rc = dalloc(e, &e->hh, (size_t)e->NS * K * P * e->esz))) return rc;
  if ((rc = dalloc(e, &e->logits, (size_t)e->NS * K * V))) return rc;
  return VC_OK;
}

// ---- the per-sequence tables of a decode step, the sampler's words and tables (and, allocated between them, the finished-row forms'
// centred copies and row means)
int alloc_seq_tables(vc_engine* e) {
  const int d = e->d, K = e->K;
  int rc;
  if ((rc = dalloc(e, &e->dec_h, (size_t)e->NS * d))) return rc;
  if ((rc = dalloc(e, &e->dec_row_seq, (size_t)e->NS))) return rc;
  if ((rc = dalloc(e, &e->dec_row_pos, (size_t)e->NS))) return rc;
  if ((rc = dalloc(e, &e->logit_row, (size_t)e->NS))) return rc;
  if ((rc = dalloc(e, &e->st, (size_t)e->NS))) return rc;
  if ((rc = dalloc(e, &e->st_fin, (size_t)e->NS))) return rc;
  if ((rc = dalloc(e, &e->hqA, (size_t)VC_ROWS * d * e->esz))) return rc;
  if ((rc = dalloc(e, &e->hqB, (size_t)VC_ROWS * d * e->esz))) return rc;
  if ((rc = dalloc0(e, &e->row_mu[0], (size_t)VC_ROWS, VC_ROWS * 4))) return rc;
  if ((rc = dalloc0(e, &e->row_mu[1], (size_t)VC_ROWS, VC_ROWS * 4))) return rc;
  if ((rc = dalloc0(e, &e->mu_zero, (size_t)VC_ROWS, VC_ROWS * 4))) return rc;
  if ((rc = dalloc0(e, &e->n_active, (size_t)4, 16))) return rc;
  if ((rc = dalloc0(e, &e->step_ctr, (size_t)4, 4))) return rc;
  if ((rc = dalloc0(e, &e->err_flag, (size_t)4, 16))) return rc;
  if ((rc = dalloc(e, &e->one, (size_t)4))) return rc;             // (set below)
  if ((rc = dalloc0(e, &e->share_len, (size_t)4, 16))) return rc;
  if ((rc = dalloc(e, &e->samp, (size_t)e->NS * (VC_MAX_CODEBOOKS + 2)))) return rc;
  if ((rc = dalloc(e, &e->cond, (size_t)e->NS))) return rc;
  if ((rc = dalloc(e, &e->amax, (size_t)e->NS))) return rc;
  if ((rc = dalloc0(e, &e->dbg_ts, (size_t)64, 64 * 8))) return rc;
  e->gen_cap = e->S_max;
  if ((rc = dalloc(e, &e->gen, (size_t)e->B_max * e->gen_cap * K))) return rc;
  { const int one[4] = {1, 1, 1, 1}; HIPCHK(e, hipMemcpy(e->one, one, 16, hipMemcpyHostToDevice)); }
  return VC_OK;
}

// ---- pinned staging of the calls; the decode sessions' tables and staging
int alloc_session_tables(vc_engine* e) {
  int rc;
  HIPCHK(e, hipHostMalloc((void**)&e->h_st, sizeof(SeqState) * e->NS));
  HIPCHK(e, hipHostMalloc((void**)&e->h_st2, sizeof(SeqState) * e->NS));
  HIPCHK(e, hipHostMalloc((void**)&e->h_flag, 64));
  memset(e->h_flag, 0, 64);
  HIPCHK(e, hipHostMalloc((void**)&e->h_dyn, sizeof(SampleDyn)));
  HIPCHK(e, hipHostMalloc((void**)&e->h_rec, sizeof(int) * VC_SESS_REC * e->NS));
  memset(e->h_rec, 0, sizeof(int) * VC_SESS_REC * e->NS);
  const size_t NS = e->NS;
  if ((rc = dalloc0(e, &e->seed_tab, NS, sizeof(uint64_t) * NS))) return rc;
  if ((rc = dalloc0(e, &e->samp_tab, NS, sizeof(int) * NS))) return rc;
  if ((rc = dalloc0(e, &e->batch_id, (size_t)4, 16))) return rc;
  if ((rc = dalloc0(e, &e->row_base, (size_t)4, 16))) return rc;
  if ((rc = dalloc0(e, &e->adm_slot, NS, sizeof(int) * NS))) return rc;
  if ((rc = dalloc0(e, &e->prompt_err, NS, sizeof(int) * NS))) return rc;
  if ((rc = dalloc(e, &e->sess_gather, NS))) return rc;
  if ((rc = dalloc0(e, &e->ctl_tab, NS, sizeof(vc_request_ctl) * NS))) return rc;
  if ((rc = dalloc0(e, &e->adm_ctl, NS, sizeof(vc_request_ctl) * NS))) return rc;
  if ((rc = dalloc0(e, &e->adm_st, NS, sizeof(SeqState) * NS))) return rc;
  HIPCHK(e, hipHostMalloc((void**)&e->h_adm_st, sizeof(SeqState) * NS * VC_ADM_STAGES));
  HIPCHK(e, hipHostMalloc((void**)&e->h_adm_ctl, sizeof(vc_request_ctl) * NS * VC_ADM_STAGES));
  if ((rc = dalloc(e, &e->d_dyn, (size_t)1))) return rc;
  return VC_OK;
}

// ---- events and streams
int make_events_streams(vc_engine* e) {
  for (auto& ev : e->ev_pace) HIPCHK(e, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  for (auto& ev : e->ev) HIPCHK(e, hipEventCreate(&ev));
  // a blocking stream: implicitly ordered after work the caller queued on the null stream
  HIPCHK(e, hipStreamCreate(&e->own_stream));
  HIPCHK(e, hipStreamCreateWithFlags(&e->side_stream, hipStreamNonBlocking));
  return VC_OK;
}

}  // namespace

extern "C" int vc_finalize_weights(vc_engine* e, int compute_dtype) {
  if (!e) return VC_EINVAL;
  if (e->finalized) return fail(e, VC_ESTATE, "already finalized");
  if (compute_dtype != VC_DTYPE_BF16 && compute_dtype != VC_DTYPE_F32) return fail(e, VC_EINVAL, "compute dtype must be bf16 or f32");
  if (e->w8_req && compute_dtype != VC_DTYPE_BF16) return fail(e, VC_EINVAL, "vc_request_w8 was made, and the w8 form exists for bf16 engines only");
  if (e->kv8_req && compute_dtype != VC_DTYPE_BF16) return fail(e, VC_EINVAL, "vc_request_kv8 was made, and the kv8 form exists for bf16 engines only");
  HIPCHK(e, hipSetDevice(e->device));
  e->dtype = compute_dtype;
  e->esz = compute_dtype == VC_DTYPE_BF16 ? 2 : 4;
  int rc;
  if ((rc = load_embeddings(e)) || (rc = load_position_table(e))) return rc;
  decide_images(e);
  e->layers.resize(e->L);
  for (int l = 0; l < e->L; ++l)
    if ((rc = pack_layer(e, l))) return rc;
  if (e->kv8_req && (rc = upload_kv8_table(e))) return rc;
  if ((rc = pack_heads(e))) return rc;
  HIPCHK(e, hipDeviceSynchronize());
  for (auto& kv : e->raw) if (kv.second.dev) (void)hipFree(kv.second.dev);
  e->raw.clear();
  make_plans(e);
  if ((rc = alloc_pass_arenas(e)) || (rc = alloc_seq_tables(e)) || (rc = alloc_session_tables(e)) || (rc = make_events_streams(e))) return rc;
  // ---- options: the VC_* environment variables preset them, vc_set_option changes them at run time
  if ((rc = apply_env_presets(e))) return rc;
  HIPCHK(e, hipDeviceSynchronize());
  e->finalized = true;
  return VC_OK;
}

// ------------------------------------------------------------------------------------- TTS
namespace {

// After a one-row-per-sequence decode loop: the final states by slot into h_st[0, B) and the call's re-pack count (host_ms[HM_REPACKS]).
// For one sequence that is the copy of its state.
int collect_states(vc_engine* e, int B, hipStream_t s) {
  if (!e->repack_at.empty()) HIPCHK(e, hipMemcpyAsync(e->h_flag + HF_LIVE_STEPS, e->step_ctr, sizeof(int), hipMemcpyDeviceToHost, s));
  if (e->cur_rows == B) {
    HIPCHK(e, hipMemcpyAsync(e->h_st, e->st, sizeof(SeqState) * B, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
  } else {      // the batch was re-packed onto fewer rows on the way: final states = the parked ones + the rows of the last layout, by slot
    const int Bc = e->cur_rows;
    HIPCHK(e, hipMemcpyAsync(e->h_st, e->st_fin, sizeof(SeqState) * B, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipMemcpyAsync(e->h_st2, e->st, sizeof(SeqState) * Bc, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    for (int r = 0; r < Bc; ++r) {
      const int slot = e->h_st2[r].slot;
      if (slot >= 0 && slot < B) e->h_st[slot] = e->h_st2[r];
    }
    const int rc = check_err_flag(e, s);
    if (rc) return rc;
  }
  // re-packs of this call: those that moved live sequences, i.e. the one queued before batch k counts when the loop's live steps
  // (step_ctr stops at the last one) reach into batch k.  Whether the host queues one more after the last sequence has retired
  // depends on how far it trails the device, so that one is not counted and the figure is the same in every run
  for (int k : e->repack_at)
    if (e->h_flag[HF_LIVE_STEPS] > k * std::max(1, e->steps_per_graph)) e->host_ms[HM_REPACKS] += 1;
  return VC_OK;
}

}  // namespace
namespace vch __attribute__((visibility("hidden"))) {
// A TTS request's prompt - one segment: the T prompt frames and the first generated column; `skip` text positions are read from
// sequence 0's cache, whose text x_shared is - and its first state.  (The blocking calls and a session's admission.)
SeqState tts_request(vc_engine* e, const TtsJob& j, int skip, const int64_t* x_shared, PromptArgs* pa) {
  fill_prompt_common(e, *pa, j.x, j.Lx, j.y, j.T);
  pa->n_seg = 1; pa->n_cols = j.T + 1;
  pa->seg[0] = Segment{0, j.T + 1, 0, j.T, -1, -1};
  pa->skip = skip; pa->x_shared = x_shared;
  return init_state(e, j.Lx, j.T + 1, true, 1);
}

// Best-of-N prefills once and replicates: the prompt positions of the entries the caller has laid down in `kv` (source and destination
// slots, position ranges), copied in every layer's K and V cache - one launch per cache tensor, whatever the number of entries.
int replicate_kv(vc_engine* e, CopyKvArgs kv, hipStream_t s) {
  const long esz = e->dtype == VC_DTYPE_BF16 ? 2 : 4;
  kv.H = e->H; kv.head_stride_b = (long)e->S_max * e->hd * esz; kv.pos_b = (long)e->hd * esz;
  kv.seq_stride_b = (long)e->H * kv.head_stride_b;
  for (int l = 0; l < e->L; ++l) {
    kv.base = (char*)e->layers[l].kc;
    HIPCHK(e, vc_launch_copy_kv(kv, s));
    kv.base = (char*)e->layers[l].vc;
    HIPCHK(e, vc_launch_copy_kv(kv, s));
  }
  if (e->kv8_req) {      // the siblings' E4M3 rows and shifts: copies of the source's, which the prefill pass packed
    CopyKvArgs k8 = kv, sh = kv;
    k8.head_stride_b = (long)e->S_max * e->hd; k8.pos_b = e->hd; k8.seq_stride_b = (long)e->H * k8.head_stride_b;
    sh.head_stride_b = (long)e->S_max * 2; sh.pos_b = 2; sh.seq_stride_b = (long)e->H * sh.head_stride_b;
    for (int l = 0; l < e->L; ++l) {
      k8.base = (char*)e->layers[l].kc8;
      HIPCHK(e, vc_launch_copy_kv(k8, s));
      k8.base = (char*)e->layers[l].vc8;
      HIPCHK(e, vc_launch_copy_kv(k8, s));
      sh.base = (char*)e->layers[l].sh8;
      HIPCHK(e, vc_launch_copy_kv(sh, s));
    }
  }
  if (e->kv8c_req) {     // ... which stand for k - c: the source's centre (and n0) goes with them, whole, whatever the position range
    CopyKvArgs cn = kv;
    cn.head_stride_b = (long)e->hd * 2; cn.pos_b = cn.head_stride_b; cn.seq_stride_b = (long)e->H * cn.head_stride_b;
    for (int i = 0; i < cn.n_ent; ++i) { cn.p0[i] = 0; cn.p1[i] = 1; }
    for (int l = 0; l < e->L; ++l) {
      cn.base = (char*)e->layers[l].kcen;
      HIPCHK(e, vc_launch_copy_kv(cn, s));
    }
    cn.H = 1; cn.head_stride_b = cn.pos_b = cn.seq_stride_b = sizeof(int);
    cn.base = (char*)e->kcen_rows;
    HIPCHK(e, vc_launch_copy_kv(cn, s));
  }
  return VC_OK;
}
}  // namespace vch
namespace {

// The blocking call's skeleton, shared by the TTS calls (tts_prepare / call_end; the streaming call too), vc_edit and vc_edit_multi:
//   call_begin - the caller's prompts and prefill, its first states into h_st[0, B) - call_arm - the decode loop - call_end.
// call_begin: every graph a call of this shape can need, captured ahead of both timers (between ev[0] and ev[1] the host
// time of capture + instantiation showed up as prefill time of a first call of a shape / option state), then ev[0].
// groups: as DecodeLoop (0, or the number of best-of-N groups).
int call_begin(vc_engine* e, int B, int rps, int groups, const vc_sample_cfg* sc, int max_steps, hipStream_t s) {
  DecodeLoop L;
  L.init(e, make_sample_args(e, B, rps), B, rps, groups, sc, max_steps, s);
  if (const int rc = L.precapture()) return rc;
  HIPCHK(e, hipEventRecord(e->ev[0], s));
  return VC_OK;
}

// call_arm: the states up, the live words set, the sampler's per-call values, the prompts' error word, and the first sample - it comes
// from the prefill logits - ahead of ev[1].  *sa: the sampler arguments the decode loop starts with.  n_group: samples per best-of-N group.
// parked: the call's loop may re-pack, so the states a re-pack parks (st_fin) are cleared.  vc_edit's one sequence never re-packs and
// its stream stays without the clear: with it bench.py --mode edit decoded 0.5 % slower (0.5459 against 0.5433 ms per step, parent spread
// 0.0005; without it 0.5433 against 0.5428, profiles/host_paths_ab.log).
int call_arm(vc_engine* e, int B, int rps, int n_group, bool parked, const vc_sample_cfg* sc, const int64_t* forced, int n_forced,
             float* logits_out, int logit_steps, hipStream_t s, SampleArgs* sa) {
  HIPCHK(e, hipMemcpyAsync(e->st, e->h_st, sizeof(SeqState) * B, hipMemcpyHostToDevice, s));
  if (parked) HIPCHK(e, hipMemsetAsync(e->st_fin, 0, sizeof(SeqState) * B, s));
  e->h_flag[HF_STAGE] = B;
  e->h_flag[HF_ACTIVE] = B;
  e->h_flag[HF_LIVE0] = B; e->h_flag[HF_LIVE1] = B;        // the two slots of "sequences still live" (SampleArgs.host_live)
  e->host_ms[HM_REPACKS] = 0;
  HIPCHK(e, hipMemcpyAsync(e->n_active, e->h_flag + HF_STAGE, sizeof(int), hipMemcpyHostToDevice, s));
  int rc = push_sample_dyn(e, sc, forced, n_forced, logits_out, logit_steps, B, s, n_group);
  if (rc) return rc;
  rc = check_err_flag(e, s);   // also orders the pinned-buffer reuse
  if (rc) return rc;
  *sa = make_sample_args(e, B, rps);
  HIPCHK(e, vc_launch_sample(*sa, n_group > 1, s));
  HIPCHK(e, hipEventRecord(e->ev[1], s));
  return VC_OK;
}

// call_end: ev[2], the final states by slot in h_st[0, B), the timings, and the steps really taken (the longest sequence; feed steps of
// an edit not counted), not the launched multiple of steps_per_graph.
int call_end(vc_engine* e, int B, bool grouped, int* steps_out, hipStream_t s) {
  HIPCHK(e, hipEventRecord(e->ev[2], s));
  int rc = collect_states(e, B, s);
  if (rc) return rc;
  if (grouped && (rc = check_err_flag(e, s))) return rc;      // the keep decisions' row check (advance_phase)
  HIPCHK(e, hipEventElapsedTime(&e->ms[0], e->ev[0], e->ev[1]));
  HIPCHK(e, hipEventElapsedTime(&e->ms[1], e->ev[1], e->ev[2]));
  e->ms[2] = e->ms[0] + e->ms[1];
  if (steps_out) {
    int m = 0;
    for (int b = 0; b < B; ++b) m = std::max(m, e->h_st[b].total_steps);
    *steps_out = m;
  }
  return VC_OK;
}

// The one TTS host path: U prompts (jobs) x n_samples (N) samples each, as U * N sequences.  Sample j of utterance u is the
// sequence of slot u * N + j and, with N > 1, a member of best-of-N group u.  vc_tts is (1, N), vc_tts_multi (U, 1) and
// vc_tts_multi_best_of (U, N).
// tts_prepare: everything up to and including the first sample (graphs pre-captured ahead of the timers, prompts, prefill, state
// upload, sampler values, the sample from the prefill logits); call_end: everything behind the decode loop (states, timing).  The
// blocking calls run prepare - decode_loop - call_end back to back (tts_run); the streaming call keeps the loop open in between.
struct TtsPrep { SampleArgs sa; int B = 0, U = 0, max_steps = 0; bool grouped = false; };
int tts_prepare(vc_engine* e, const std::vector<TtsJob>& jobs, int n_samples, const vc_sample_cfg* sc,
                const int64_t* forced, int n_forced, float* logits_out, int logit_steps,
                hipStream_t s, int shared_prefix, TtsPrep* prep, bool* share_armed) {
  const int K = e->K;
  const int U = (int)jobs.size(), N = n_samples;
  if (N < 1) return fail(e, VC_EINVAL, "n_samples %d must be at least 1", N);
  const bool grouped = N > 1;
  const int B = U * N;
  if (B > e->B_max) {
    if (grouped && U > 1)
      return fail(e, VC_ECAP, "%d sequences requested (%d utterances x %d samples) but max_seqs is %d", B, U, N, e->B_max);
    return fail(e, VC_ECAP, "%d sequences requested but max_seqs is %d", B, e->B_max);
  }
  int max_steps = 0;
  for (int b = 0; b < U; ++b) {
    const TtsJob& j = jobs[b];
    if (j.Lx < 1 || j.T < 0) return fail(e, VC_EINVAL, "empty text or negative prompt length");
    const int n_cols = j.T + 1;                           // T+K columns minus the K-1 dropped ones (:967)
    const int cap_len = j.Lx * (e->cfg.encodec_sr / 5);
    int steps = std::max(0, cap_len - n_cols + 1) + K;
    // The reference grows its cache as it goes and normally stops at the terminator long before the
    // length cap (voicecraft.py:1041-1045), so the worst case is not required to fit: the step budget
    // is clamped to the room there is, the in-kernel capacity guard (vc_tokens.hip advance_phase) ends a
    // sequence that really runs out of positions, and only that case is reported (VC_ECAP, below).
    const int room = e->S_max - (j.Lx + n_cols) - 1;
    if (room < K + 1)
      return fail(e, VC_ECAP, "sequence %d: the prompt alone takes %d of max_positions %d", b, j.Lx + n_cols, e->S_max);
    steps = std::min(steps, room);
    max_steps = std::max(max_steps, steps);
  }
  max_steps = std::min(max_steps, e->gen_cap);
  if (const int rc0 = call_begin(e, B, 1, grouped ? U : 0, sc, max_steps, s)) return rc0;
  // ---- prompts + ONE prefill over all of them, into the slots of the groups' first samples
  {
    std::vector<PromptArgs> pas(U);
    std::vector<int> slots(U);
    for (int u = 0; u < U; ++u) {
      const TtsJob& j = jobs[u];
      // the shared text prefix is prefilled once, in sequence 0, and checked on the device to be the same text (prompt_k)
      e->h_st[u * N] = tts_request(e, j, (u > 0) ? shared_prefix : 0, jobs[0].x, &pas[u]);
      slots[u] = u * N;
      e->h_st[u * N].slot = u * N;
    }
    e->h_flag[HF_SHARE] = shared_prefix;
    HIPCHK(e, hipMemcpyAsync(e->share_len, e->h_flag + HF_SHARE, sizeof(int), hipMemcpyHostToDevice, s));
    *share_armed = shared_prefix > 0;
    int rc = prefill_batch(e, pas, slots, s);
    if (rc) return rc;
  }
  if (grouped) {
    // best-of-N prefills once per group and replicates: every sample starts from its prompt's K/V and first-step logits.  Positions
    // below the shared prefix are read from sequence 0's cache by every sequence, so they are not copied.  One launch per cache tensor
    // and one for the logits, whatever the number of groups
    CopyKvArgs kv;
    memset(&kv, 0, sizeof kv);
    kv.n_ent = U; kv.n_dst = U * (N - 1);
    for (int u = 0; u < U; ++u) {
      kv.src[u] = u * N; kv.dst0[u] = u * N + 1; kv.cnt[u] = N - 1;
      kv.p0[u] = shared_prefix; kv.p1[u] = jobs[u].Lx + jobs[u].T + 1;
    }
    CopyKvArgs lg = kv;
    if (const int rc = replicate_kv(e, kv, s)) return rc;
    lg.base = (char*)e->logits; lg.H = 1; lg.seq_stride_b = lg.pos_b = (long)K * e->V * 4;
    for (int u = 0; u < U; ++u) { lg.p0[u] = 0; lg.p1[u] = 1; }
    HIPCHK(e, vc_launch_copy_kv(lg, s));
    for (int u = 0; u < U; ++u)
      for (int j = 0; j < N; ++j) {
        SeqState& st = e->h_st[u * N + j];
        if (j > 0) st = e->h_st[u * N];
        st.slot = u * N + j;
        st.group = u;
      }
  }
  if (const int rc = call_arm(e, B, 1, N, true, sc, forced, n_forced, logits_out, logit_steps, s, &prep->sa)) return rc;
  prep->B = B; prep->U = U; prep->max_steps = max_steps; prep->grouped = grouped;
  return VC_OK;
}

int tts_run(vc_engine* e, const std::vector<TtsJob>& jobs, int n_samples, const vc_sample_cfg* sc,
            const int64_t* forced, int n_forced, float* logits_out, int logit_steps, int* steps_out,
            hipStream_t s, int shared_prefix = 0) {
  // the device word share_len is non-zero only inside this call, whichever way it ends (a later vc_eval_forward or
  // vc_edit would otherwise read positions below it from sequence 0's cache)
  struct ShareGuard {
    vc_engine* e; hipStream_t s; bool armed = false;
    ~ShareGuard() { if (armed) (void)hipMemsetAsync(e->share_len, 0, sizeof(int), s); }
  } share_guard{e, s};
  TtsPrep prep;
  int rc = tts_prepare(e, jobs, n_samples, sc, forced, n_forced, logits_out, logit_steps, s, shared_prefix, &prep, &share_guard.armed);
  if (rc) return rc;
  rc = decode_loop(e, prep.sa, prep.B, 1, prep.grouped ? prep.U : 0, sc, prep.max_steps, s);
  if (rc) return rc;
  return call_end(e, prep.B, prep.grouped, steps_out, s);
}

// The sample utterance u of a tts_run keeps: the member that is kept, done and has its span (-1 if none terminated).
int kept_sample(const vc_engine* e, int u, int N) {
  int keep = -1;
  for (int j = 0; j < N; ++j) {
    const SeqState& st = e->h_st[u * N + j];
    if (st.kept && st.done && st.span >= 1) keep = j;
  }
  return keep;
}

}  // namespace
namespace vch __attribute__((visibility("hidden"))) {
// (st: the sequence's final state - the blocking calls read it back into h_st, a session rebuilds what is needed from the slot's record)
int assemble_tts(vc_engine* e, const TtsJob& j, int slot, const SeqState& st, int64_t* res, int res_cap, int* gen_len, hipStream_t s) {
  if (!st.done || st.span < 1)
    return fail(e, VC_ECAP, "generation ran out of room before it terminated (max_positions %d): raise max_positions", e->S_max);
  const int N = st.span_steps[0];
  const int Tg = N - e->K;                                  // voicecraft.py:1137
  if (Tg < 0) return fail(e, VC_ESTATE, "internal: span of %d steps", N);
  if (j.T + Tg > res_cap) return fail(e, VC_ECAP, "res capacity %d < %d", res_cap, j.T + Tg);
  AssembleArgs a;
  memset(&a, 0, sizeof a);
  a.y = j.y; a.gen = e->gen + (size_t)slot * e->gen_cap * e->K; a.K = e->K; a.T = j.T; a.res_cap = res_cap; a.res = res;
  a.n_piece = 0;
  if (j.T > 0) { a.kind[a.n_piece] = 0; a.src0[a.n_piece] = 0; a.len[a.n_piece] = j.T; a.dst0[a.n_piece] = 0; a.n_piece++; }
  if (Tg > 0) { a.kind[a.n_piece] = 1; a.src0[a.n_piece] = 0; a.len[a.n_piece] = Tg; a.dst0[a.n_piece] = j.T; a.n_piece++; }
  HIPCHK(e, vc_launch_assemble(a, s));
  *gen_len = Tg;
  return VC_OK;
}
}  // namespace vch

// ---- the streaming TTS call: tts_prepare at begin, the DecodeLoop advanced from next, call_end + assemble_tts at end
struct TtsStream {
  TtsJob job{};
  TtsPrep prep{};
  DecodeLoop L{};
  hipStream_t s = nullptr;
  int emitted = 0;          // frames handed out so far
  bool finished = false;    // call_end has run: h_st[0] holds the final state
  int finish_rc = VC_OK;
  int Tg = -1;              // generated frames, known once finished (-1: the sequence did not terminate)
  int n_steps = 0;
};
namespace {
void drop_tts_stream(vc_engine* e) {
  delete e->ts;
  e->ts = nullptr;
}

// once the loop is over: the blocking call's tail (states, timing); the frame count then comes from the sequence's state
int stream_finalize(vc_engine* e) {
  TtsStream& t = *e->ts;
  if (t.finished) return t.finish_rc;
  t.L.finish(nullptr);
  t.finish_rc = call_end(e, t.prep.B, t.prep.grouped, &t.n_steps, t.s);
  t.finished = true;
  const SeqState& st = e->h_st[0];
  if (t.finish_rc == VC_OK && st.done && st.span >= 1) t.Tg = std::max(0, st.span_steps[0] - e->K);
  return t.finish_rc;
}

// frames [t.emitted, ...) that `rows` finished rows of the gen buffer hold, un-shifted into the caller's block on the side stream
int stream_gather(vc_engine* e, int rows, int64_t* codes, int cap, int* n_out) {
  TtsStream& t = *e->ts;
  StreamGatherArgs a;
  memset(&a, 0, sizeof a);
  a.st = e->st; a.gen = e->gen; a.K = e->K; a.rows = rows; a.first = t.emitted; a.cap = cap; a.out = codes; a.host_n = e->h_flag + HF_GATHER_N;
  e->h_flag[HF_GATHER_N] = 0;
  HIPCHK(e, vc_launch_stream_gather(a, e->side_stream));
  HIPCHK(e, hipStreamSynchronize(e->side_stream));       // the side stream only: the decode stream's queued graphs are not waited for
  *n_out = e->h_flag[HF_GATHER_N];
  return VC_OK;
}
}  // namespace

extern "C" int vc_tts_stream_begin(vc_engine* e, const int64_t* x_dev, int Lx, const int64_t* y_dev, int T,
                                   const vc_sample_cfg* sc, const int64_t* forced_dev, int n_forced, void* stream) {
  if (!x_dev || (!y_dev && T > 0) || !sc || Lx < 1 || T < 0 || n_forced < 0)
    return fail(e, VC_EINVAL, "null/invalid argument to vc_tts_stream_begin");
  int rc = check_idle(e);
  if (rc) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : e->own_stream;
  std::vector<TtsJob> jobs{TtsJob{x_dev, Lx, y_dev, T}};
  TtsPrep prep;
  bool share_armed = false;
  rc = tts_prepare(e, jobs, 1, sc, forced_dev, n_forced, nullptr, 0, s, 0, &prep, &share_armed);
  if (rc) return rc;
  TtsStream* t = new TtsStream();
  t->job = jobs[0]; t->prep = prep; t->s = s;
  t->L.init(e, prep.sa, prep.B, 1, 0, sc, prep.max_steps, s);
  e->ts = t;
  rc = t->L.begin();
  if (rc) drop_tts_stream(e);
  return rc;
}

extern "C" int vc_tts_stream_next(vc_engine* e, int min_frames, int64_t* codes_dev, int cap, int* first_frame, int* n_frames,
                                  int* done) {
  if (!codes_dev || cap < 1 || min_frames < 1 || min_frames > cap || !first_frame || !n_frames || !done)
    return fail(e, VC_EINVAL, "null/invalid argument to vc_tts_stream_next (min_frames %d, cap %d)", min_frames, cap);
  if (!e) return VC_EINVAL;
  if (!e->ts) return fail(e, VC_ESTATE, "no streaming TTS call is open (vc_tts_stream_begin)");
  HIPCHK(e, hipSetDevice(e->device));
  TtsStream& t = *e->ts;
  const int K = e->K;
  for (;;) {
    int rc, n = 0;
    if (t.L.over) {
      // the sequence has ended (or the step budget has): the count comes from its state, never from the launched multiple of graph_steps
      if ((rc = stream_finalize(e))) return rc;
      if (t.Tg > t.emitted && (rc = stream_gather(e, t.Tg + K, codes_dev, cap, &n))) return rc;
      *first_frame = t.emitted; *n_frames = n;
      t.emitted += n;
      *done = t.emitted >= t.Tg;
      return VC_OK;
    }
    // a live sequence: after S finished rows (the first sample + the steps whose pacing event has been waited for), frames
    // < S - (K - 1) are complete (out[j][t] = rows[j + t][j]).  The kernel clamps the count to the sequence's own state.
    const int rows = 1 + t.L.complete;
    if (rows - (K - 1) - t.emitted >= min_frames) {
      if ((rc = stream_gather(e, rows, codes_dev, cap, &n))) return rc;
      if (n >= min_frames) {
        *first_frame = t.emitted; *n_frames = n; *done = 0;
        t.emitted += n;
        return VC_OK;
      }
    }
    if ((rc = t.L.advance())) return rc;
  }
}

extern "C" int vc_tts_stream_end(vc_engine* e, int64_t* res_dev, int res_cap, int* gen_len, int* n_steps) {
  if (res_dev && (!gen_len || res_cap < 0)) return fail(e, VC_EINVAL, "null/invalid argument to vc_tts_stream_end");
  if (!e) return VC_EINVAL;
  if (!e->ts) return fail(e, VC_ESTATE, "no streaming TTS call is open (vc_tts_stream_begin)");
  HIPCHK(e, hipSetDevice(e->device));
  TtsStream& t = *e->ts;
  int rc = VC_OK;
  if (!res_dev) {             // abort: wait for what is queued; the next call uploads every state afresh
    if (!t.finished) {
      t.L.finish(nullptr);
      hipError_t se = hipStreamSynchronize(t.s);
      if (se != hipSuccess) rc = fail(e, VC_EHIP, "hipStreamSynchronize: %s", hipGetErrorString(se));
    }
    drop_tts_stream(e);
    return rc;
  }
  while (rc == VC_OK && !t.L.over) rc = t.L.advance();
  if (rc == VC_OK) rc = stream_finalize(e);
  if (rc == VC_OK) rc = assemble_tts(e, t.job, 0, e->h_st[0], res_dev, res_cap, gen_len, t.s);
  if (rc == VC_OK) {
    hipError_t se = hipStreamSynchronize(t.s);
    if (se != hipSuccess) rc = fail(e, VC_EHIP, "hipStreamSynchronize: %s", hipGetErrorString(se));
  }
  if (rc == VC_OK && n_steps) *n_steps = t.n_steps;
  drop_tts_stream(e);
  return rc;
}

// ------------------------------------------------------------------------------------- editing: the parts shared by vc_edit, vc_edit_multi and the decode sessions
namespace vch __attribute__((visibility("hidden"))) {

// Validation, segment table and step budget of one request (vc_edit, vc_edit_multi; `who` prefixes every message).
int edit_prepare(vc_engine* e, EditJob& j, const char* who) {
  const int K = e->K, M = j.M, Lx = j.Lx, T = j.T;
  const vc_model_cfg& c = e->cfg;
  if (M < 1 || M > c.max_n_spans || 2 * M + 1 > VC_MAX_SPANS * 2 + 1)
    return fail(e, VC_EINVAL, "%snumber of spans %d outside [1,%d]", who, M, c.max_n_spans);
  if (Lx < 1 || T < 1) return fail(e, VC_EINVAL, "%sempty text or audio", who);
  if (c.eos > 0 && !c.reduced_eog) return fail(e, VC_EINVAL, "%seos > 0 requires reduced_eog (voicecraft.py:244)", who);
  // non-mask intervals (voicecraft.py:620-628)
  std::vector<int>& ns = j.ns;
  std::vector<int>& ne = j.ne;
  ns.assign(M + 1, 0); ne.assign(M + 1, 0);
  for (int i = 0; i <= M; ++i) {
    ns[i] = (i == 0) ? 0 : j.iv[2 * (i - 1) + 1];
    ne[i] = (i == M) ? T : j.iv[2 * i];
    if (ns[i] < 0 || ne[i] > T || ne[i] < ns[i])
      return fail(e, VC_EINVAL, "%smask intervals must be ordered, disjoint and inside [0,%d]", who, T);
  }
  for (int i = 0; i < M; ++i)
    if (j.iv[2 * i + 1] < j.iv[2 * i]) return fail(e, VC_EINVAL, "%smask interval %d is reversed", who, i);
  for (int i = 0; i < 2 * M; ++i)
    if (j.mv[i] < 0 || j.mv[i] >= c.max_n_spans) return fail(e, VC_EINVAL, "%smask value out of range", who);
  // segments of the prefill: every non-mask piece (delay-shifted, K extra columns), a mask
  // placeholder after each of them, and the first all-empty column of the first masked piece
  // (rearrange :239-252, shift :254-262, insert_mask :264-288, the cut at :672-679)
  PromptArgs& pa = j.pa;
  fill_prompt_common(e, pa, j.x, Lx, j.y, T);
  int col = 0, nseg = 0;
  for (int i = 0; i <= M; ++i) {
    int term = -1;
    if (c.eos > 0) term = (i == M) ? c.eos : -1;
    else if (c.reduced_eog) term = (i == M) ? c.eog : -1;
    else term = c.eog;
    const int n = (ne[i] - ns[i]) + (term >= 0 ? 1 : 0);
    if (n <= 0)   // the reference raises IndexError here (codebooks_patterns.py:174 on a zero-length piece)
      return fail(e, VC_EINVAL, "%snon-masked piece %d is empty (a span may not start at frame 0)", who, i);
    pa.seg[nseg++] = Segment{col, n + K, ns[i], ne[i] - ns[i], term, -1};
    col += n + K;
    pa.seg[nseg++] = Segment{col, 1, 0, 0, -1, j.mv[i]};
    col += 1;
  }
  pa.seg[nseg++] = Segment{col, 1, 0, 0, -1, -1};   // s = 0 of the first masked piece: all `empty`
  col += 1;
  pa.n_seg = nseg; pa.n_cols = col;
  const int cap_len = Lx * 10;
  int max_steps = std::max(0, cap_len - col + 1) + M * (K + 4) + 8;
  {   // as in tts_run: clamp to the room there is; running out of it is reported after the loop
    const int room = e->S_max - (Lx + col) - 3 * M - 1;
    if (room < M * (K + 1))
      return fail(e, VC_ECAP, "%sediting: the rearranged prompt alone takes %d of max_positions %d", who, Lx + col, e->S_max);
    max_steps = std::min(std::min(max_steps, room), e->gen_cap);
  }
  j.max_steps = max_steps;
  return VC_OK;
}

// The request's first state: more_mask_value (:676) per span switch.
SeqState edit_state(vc_engine* e, const EditJob& j) {
  SeqState st = init_state(e, j.Lx, j.pa.n_cols, false, j.M);
  for (int i = 1; i < j.M; ++i) st.mask_value[i] = j.mv[j.M + i];
  return st;
}

// res = nonmask_0, gen_0, nonmask_1, gen_1, ..., nonmask_M (voicecraft.py:890-898) from the request's final state and gen rows.
int edit_assemble(vc_engine* e, const EditJob& j, const SeqState& fs, const int* gen, int64_t* res, int res_cap, int* res_len,
                  hipStream_t s, const char* who) {
  const int K = e->K, M = j.M;
  if (!fs.done || fs.span < M)
    return fail(e, VC_ECAP, "%sediting ran out of room before it terminated (max_positions %d): raise max_positions", who, e->S_max);
  AssembleArgs a;
  memset(&a, 0, sizeof a);
  a.y = j.y; a.gen = gen; a.K = K; a.T = j.T; a.res_cap = res_cap; a.res = res;
  int dst = 0, g0 = 0;
  for (int i = 0; i <= M; ++i) {
    if (j.ne[i] > j.ns[i]) { int p = a.n_piece++; a.kind[p] = 0; a.src0[p] = j.ns[i]; a.len[p] = j.ne[i] - j.ns[i]; a.dst0[p] = dst; dst += j.ne[i] - j.ns[i]; }
    if (i < M) {
      const int N = fs.span_steps[i], Tg = N - K;
      if (Tg < 0) return fail(e, VC_ESTATE, "%sinternal: span of %d steps", who, N);
      if (Tg > 0) { int p = a.n_piece++; a.kind[p] = 1; a.src0[p] = g0; a.len[p] = Tg; a.dst0[p] = dst; dst += Tg; }
      g0 += N;
    }
  }
  if (dst > res_cap) return fail(e, VC_ECAP, "%sres capacity %d < %d", who, res_cap, dst);
  HIPCHK(e, vc_launch_assemble(a, s));
  *res_len = dst;
  return VC_OK;
}

}  // namespace vch

extern "C" int vc_tts(vc_engine* e, const int64_t* x_dev, int Lx, const int64_t* y_dev, int T,
                      const vc_sample_cfg* sc, int n_samples, const int64_t* forced_dev, int n_forced,
                      int64_t* res_dev, int res_cap, int* gen_len, float* logits_dev, int logit_steps,
                      int* n_steps, void* stream) {
  int rc = check_idle(e);
  if (rc) return rc;
  if (!x_dev || (!y_dev && T > 0) || !sc || !res_dev || !gen_len || n_samples < 1)
    return fail(e, VC_EINVAL, "null/invalid argument to vc_tts");
  hipStream_t s = stream ? (hipStream_t)stream : e->own_stream;
  std::vector<TtsJob> jobs{TtsJob{x_dev, Lx, y_dev, T}};
  rc = tts_run(e, jobs, n_samples, sc, forced_dev, n_forced, logits_dev, logit_steps, n_steps, s);
  if (rc) return rc;
  int slot = 0;
  if (n_samples > 1) {
    slot = kept_sample(e, 0, n_samples);
    if (slot < 0) return fail(e, VC_ECAP, "no sample terminated within the step budget");
  }
  rc = assemble_tts(e, jobs[0], slot, e->h_st[slot], res_dev, res_cap, gen_len, s);
  if (rc) return rc;
  HIPCHK(e, hipStreamSynchronize(s));
  return VC_OK;
}

extern "C" int vc_tts_multi_best_of(vc_engine* e, int B, int n_samples, const int64_t* x_dev, const int32_t* x_off,
                                    const int64_t* y_dev, const int32_t* y_off, const vc_sample_cfg* sc, int shared_text_prefix,
                                    const int64_t* forced_dev, int n_forced, int64_t* res_dev, int res_cap, int* gen_len,
                                    int* kept, float* logits_dev, int logit_steps, int* n_steps, void* stream) {
  int rc = check_idle(e);
  if (rc) return rc;
  if (B < 1 || n_samples < 1 || !x_dev || !x_off || !y_dev || !y_off || !sc || !res_dev || !gen_len)
    return fail(e, VC_EINVAL, "null/invalid argument to vc_tts_multi (B %d, n_samples %d)", B, n_samples);
  for (int b = 0; b < B; ++b)
    if (shared_text_prefix < 0 || shared_text_prefix >= x_off[b + 1] - x_off[b])
      return fail(e, VC_EINVAL, "shared_text_prefix %d must be shorter than every text (sequence %d has %d tokens)",
                  shared_text_prefix, b, x_off[b + 1] - x_off[b]);
  hipStream_t s = stream ? (hipStream_t)stream : e->own_stream;
  std::vector<TtsJob> jobs;
  for (int b = 0; b < B; ++b)
    jobs.push_back(TtsJob{x_dev + x_off[b], x_off[b + 1] - x_off[b], y_dev + (size_t)y_off[b] * e->K, y_off[b + 1] - y_off[b]});
  rc = tts_run(e, jobs, n_samples, sc, forced_dev, n_forced, logits_dev, logit_steps, n_steps, s, B > 1 ? shared_text_prefix : 0);
  if (rc) return rc;
  for (int b = 0; b < B; ++b) {
    const int j = n_samples > 1 ? kept_sample(e, b, n_samples) : 0;
    if (j < 0) return fail(e, VC_ECAP, "utterance %d: no sample terminated within the step budget", b);
    if (kept) kept[b] = j;
    const SeqState& st = e->h_st[b * n_samples + j];
    rc = assemble_tts(e, jobs[b], b * n_samples + j, st, res_dev + (size_t)b * e->K * res_cap, res_cap, &gen_len[b], s);
    if (rc) return rc;
  }
  HIPCHK(e, hipStreamSynchronize(s));
  return VC_OK;
}

extern "C" int vc_tts_multi(vc_engine* e, int B, const int64_t* x_dev, const int32_t* x_off,
                            const int64_t* y_dev, const int32_t* y_off, const vc_sample_cfg* sc,
                            int shared_text_prefix,
                            const int64_t* forced_dev, int n_forced, int64_t* res_dev, int res_cap, int* gen_len,
                            float* logits_dev, int logit_steps, int* n_steps, void* stream) {
  return vc_tts_multi_best_of(e, B, 1, x_dev, x_off, y_dev, y_off, sc, shared_text_prefix, forced_dev, n_forced, res_dev, res_cap,
                              gen_len, nullptr, logits_dev, logit_steps, n_steps, stream);
}

// ------------------------------------------------------------------------------------- editing (EditJob, edit_prepare, edit_state, edit_assemble: above the decode sessions)
extern "C" int vc_edit(vc_engine* e, const int64_t* x_dev, int Lx, const int64_t* y_dev, int T,
                       const int32_t* mask_intervals, int M, const int32_t* mask_values,
                       const vc_sample_cfg* sc, const int64_t* forced_dev, int n_forced,
                       int64_t* res_dev, int res_cap, int* res_len, float* logits_dev, int logit_steps,
                       int* n_steps, void* stream) {
  int rc = check_idle(e);
  if (rc) return rc;
  if (!x_dev || !y_dev || !mask_intervals || !mask_values || !sc || !res_dev || !res_len)
    return fail(e, VC_EINVAL, "null argument to vc_edit");
  EditJob j{x_dev, Lx, y_dev, T, mask_intervals, M, mask_values};
  if ((rc = edit_prepare(e, j, ""))) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : e->own_stream;
  const int rps = (M > 1) ? 3 : 1;      // a span switch is one 3-row step (vc_edit_multi feeds it over three one-row steps instead)
  if ((rc = call_begin(e, 1, rps, 0, sc, j.max_steps, s))) return rc;
  std::vector<PromptArgs> pas(1, j.pa);
  if ((rc = prefill_batch(e, pas, std::vector<int>(1, 0), s))) return rc;
  e->h_st[0] = edit_state(e, j);
  SampleArgs sa;
  if ((rc = call_arm(e, 1, rps, 1, false, sc, forced_dev, n_forced, logits_dev, logit_steps, s, &sa))) return rc;
  if ((rc = decode_loop(e, sa, 1, rps, 0, sc, j.max_steps, s))) return rc;
  if ((rc = call_end(e, 1, false, n_steps, s))) return rc;
  rc = edit_assemble(e, j, e->h_st[0], e->gen, res_dev, res_cap, res_len, s, "");
  if (rc) return rc;
  HIPCHK(e, hipStreamSynchronize(s));
  return VC_OK;
}

// B editing requests as one batch: ONE prefill over all their prompts, then one decode row per request.  A span switch is fed as
// three one-row steps (SeqState.feed_switch, vc_tokens.hip advance_phase) instead of vc_edit's 3-row step, so a step stays B rows
// wide and the batch re-packs onto narrower steps as requests retire, as in vc_tts_multi.
extern "C" int vc_edit_multi(vc_engine* e, int B, const int64_t* x_dev, const int32_t* x_off,
                             const int64_t* y_dev, const int32_t* y_off,
                             const int32_t* mask_intervals, const int32_t* span_off, const int32_t* mask_values,
                             const vc_sample_cfg* sc, const int64_t* forced_dev, int n_forced,
                             int64_t* res_dev, int res_cap, int* res_len, float* logits_dev, int logit_steps,
                             int* n_steps, void* stream) {
  int rc = check_idle(e);
  if (rc) return rc;
  if (B < 1 || !x_dev || !x_off || !y_dev || !y_off || !mask_intervals || !span_off || !mask_values || !sc || !res_dev || !res_len)
    return fail(e, VC_EINVAL, "null/invalid argument to vc_edit_multi");
  if (B > e->B_max) return fail(e, VC_ECAP, "%d requests, the engine was created for max_seqs %d", B, e->B_max);
  const int K = e->K;
  std::vector<EditJob> jobs(B);
  std::vector<std::string> who(B);
  int loop_steps = 0;
  for (int b = 0; b < B; ++b) {
    char buf[32];
    snprintf(buf, sizeof buf, "request %d: ", b);
    who[b] = buf;
    if (x_off[b] < 0 || y_off[b] < 0 || span_off[b] < 0) return fail(e, VC_EINVAL, "%snegative offset", buf);
    EditJob& j = jobs[b];
    j.x = x_dev + x_off[b]; j.Lx = x_off[b + 1] - x_off[b];
    j.y = y_dev + (size_t)y_off[b] * K; j.T = y_off[b + 1] - y_off[b];
    j.iv = mask_intervals + 2 * (size_t)span_off[b]; j.M = span_off[b + 1] - span_off[b];
    j.mv = mask_values + 2 * (size_t)span_off[b];
    if ((rc = edit_prepare(e, j, buf))) return rc;
    loop_steps = std::max(loop_steps, j.max_steps + 2 * (j.M - 1));     // + the two feed steps of every span switch
  }
  hipStream_t s = stream ? (hipStream_t)stream : e->own_stream;
  // (the graphs of width B and of the narrower widths a shrinking batch passes through)
  if ((rc = call_begin(e, B, 1, 0, sc, loop_steps, s))) return rc;
  std::vector<PromptArgs> pas(B);
  std::vector<int> slots(B);
  for (int b = 0; b < B; ++b) { pas[b] = jobs[b].pa; slots[b] = b; }
  if ((rc = prefill_batch(e, pas, slots, s))) return rc;
  for (int b = 0; b < B; ++b) {
    e->h_st[b] = edit_state(e, jobs[b]);
    e->h_st[b].slot = b;
    e->h_st[b].feed_switch = 1;
  }
  SampleArgs sa;
  if ((rc = call_arm(e, B, 1, 1, true, sc, forced_dev, n_forced, logits_dev, logit_steps, s, &sa))) return rc;
  if ((rc = decode_loop(e, sa, B, 1, 0, sc, loop_steps, s))) return rc;
  if ((rc = call_end(e, B, false, n_steps, s))) return rc;
  for (int b = 0; b < B; ++b) {
    rc = edit_assemble(e, jobs[b], e->h_st[b], e->gen + (size_t)b * e->gen_cap * K, res_dev + (size_t)b * K * res_cap, res_cap,
                       &res_len[b], s, who[b].c_str());
    if (rc) return rc;
  }
  HIPCHK(e, hipStreamSynchronize(s));
  return VC_OK;
}

// ------------------------------------------------------------------------------------- hooks
namespace {
// vc_debug_read "<form>_stats": int32 {state (0 not applicable, 1 packed, 2 refused), fragments or pairs refused} of every slot the
// name covers, layer by layer.  false: no such buffer on this engine.
//   w13_stats, w8_stats   [layer][FFN-down, QKV]: the group planes (w8: all 0 on an engine without vc_request_w8)
//   w8w_stats             [layer][FFN-down, QKV]: the pair planes of the 16-channel images, on engines with vc_request_w8_wide
//   w8u_stats, w8ur_stats [layer]: the pair planes of W1 - one slot, the planes are shared -, on engines with vc_request_w8_up / _up_rows
//   w8q_stats             [layer]: the pairs of the 12-channel QKV image, on engines with vc_request_w8_qkv_rows (layer 0: 0, 0)
bool pack_stats(const vc_engine* e, const std::string& n, std::vector<int32_t>& v) {
  const int kind = n == "w13_stats" ? VC_PK_W13 : n == "w8_stats" ? VC_PK_W8 : n == "w8w_stats" && e->w8w_req ? PK_W8W : -1;
  const bool up = (n == "w8u_stats" && e->w8u_req) || (n == "w8ur_stats" && e->w8ur_req), q12 = n == "w8q_stats" && e->w8q_req;
  if (kind < 0 && !up && !q12) return false;
  auto put = [&](const Layer::Packed& p) { v.push_back(p.state); v.push_back(p.refused); };
  for (const Layer& ly : e->layers) {
    if (kind >= 0) { put(ly.packed[kind][W13_F2]); put(ly.packed[kind][W13_QKV]); }
    else put(up ? ly.packed[PK_W8W][W13_F1] : ly.w8q);
  }
  return true;
}
}  // namespace
extern "C" int vc_debug_read(vc_engine* e, const char* name, void* host_dst, int64_t nbytes) {
  int rc = check_ready(e);
  if (rc) return rc;
  const void* src = nullptr;
  const void* host_src = nullptr;
  int64_t avail = 0;
  const std::string n = name ? name : "";
  if (n == "logits") { src = e->logits; avail = (int64_t)e->NS * e->K * e->V * 4; }
  else if (n == "hA") { src = e->hA; avail = (int64_t)VC_ROWS * e->d * 4; }
  else if (n == "hB") { src = e->hB; avail = (int64_t)VC_ROWS * e->d * 4; }
  else if (n == "q") { src = e->q; avail = (int64_t)VC_ROWS * e->d * 4; }
  else if (n == "parts") { src = e->parts; avail = (int64_t)VC_MAX_KSPLIT * VC_SLAB_ROWS * e->d * 4; }
  else if (n == "emb") { src = e->emb; avail = (int64_t)e->emb_cap * e->d * 4; }
  else if (n == "dec_h") { src = e->dec_h; avail = (int64_t)e->NS * e->d * 4; }
  else if (n == "gen") { src = e->gen; avail = (int64_t)e->B_max * e->gen_cap * e->K * 4; }
  else if (n == "state") { src = e->st; avail = (int64_t)sizeof(SeqState) * e->NS; }
  else if ((n.rfind("kcache", 0) == 0 || n.rfind("vcache", 0) == 0) && n.size() > 6 && n.size() <= 9 &&
           n.find_first_not_of("0123456789", 6) == std::string::npos && atoi(n.c_str() + 6) < e->L) {      // kcache<l> / vcache<l>: [max_seqs][H][max_positions][hd]
    const Layer& ly = e->layers[atoi(n.c_str() + 6)];
    src = n[0] == 'k' ? ly.kc : ly.vc; avail = (int64_t)e->B_max * e->H * e->S_max * e->hd * e->esz;
  }
  else if ((n.rfind("kcache8_", 0) == 0 || n.rfind("vcache8_", 0) == 0 || n.rfind("kvshift8_", 0) == 0) && e->kv8_req) {
    // kcache8_<l> / vcache8_<l>: uint8 [max_seqs][H][max_positions][hd]; kvshift8_<l>: int8 [max_seqs][H][max_positions][2] (engines with vc_request_kv8)
    const size_t at = n.find('_') + 1;
    if (at >= n.size() || n.size() > at + 3 || n.find_first_not_of("0123456789", at) != std::string::npos || atoi(n.c_str() + at) >= e->L)
      return fail(e, VC_EINVAL, "unknown debug buffer '%s'", n.c_str());
    const Layer& ly = e->layers[atoi(n.c_str() + at)];
    const int64_t rows = (int64_t)e->B_max * e->H * e->S_max;
    if (n[1] == 'v') { src = ly.sh8; avail = rows * 2; }
    else { src = n[0] == 'k' ? ly.kc8 : ly.vc8; avail = rows * e->hd; }
  }
  else if (n.rfind("kcentre_", 0) == 0 && e->kv8c_req) {      // kcentre_<l>: bf16 [max_seqs][H][hd]; kcentre_rows: int32 [max_seqs] (engines with vc_request_kv8c)
    if (n == "kcentre_rows") { src = e->kcen_rows; avail = (int64_t)e->B_max * 4; }
    else {
      if (n.size() < 9 || n.size() > 11 || n.find_first_not_of("0123456789", 8) != std::string::npos || atoi(n.c_str() + 8) >= e->L)
        return fail(e, VC_EINVAL, "unknown debug buffer '%s'", n.c_str());
      src = e->layers[atoi(n.c_str() + 8)].kcen; avail = (int64_t)e->B_max * e->H * e->hd * 2;
    }
  }
  else if ((n.rfind("w8q_planes_", 0) == 0 || n.rfind("w8q_side_", 0) == 0) && e->w8q_req) {      // w8q_planes_<l>: uint8 [pairs][768], w8q_side_<l>: uint8 [pairs][2] of a packed layer (engines with vc_request_w8_qkv_rows)
    const bool planes = n[4] == 'p';
    const size_t at = planes ? 11 : 9;
    if (at >= n.size() || n.size() > at + 3 || n.find_first_not_of("0123456789", at) != std::string::npos || atoi(n.c_str() + at) >= e->L)
      return fail(e, VC_EINVAL, "unknown debug buffer '%s'", n.c_str());
    const Layer& ly = e->layers[atoi(n.c_str() + at)];
    if (ly.w8q.state != 1) return fail(e, VC_ESTATE, "debug buffer '%s': the layer holds no pairs of the 12-channel QKV image", n.c_str());
    const int64_t pairs = (int64_t)(3 * e->d / VC_TH_QKV) * (e->d / 64);
    if (planes) { src = ly.w8q.planes; avail = pairs * VC_W8Q_PAIR_BYTES; }
    else { src = ly.w8q.side; avail = pairs * 2; }
  }
  else if (n == "eval_logits") {                    // fp32 [rows][K][V] of the last vc_eval_forward call with the parity hook
    if (!e->eval_logits) return fail(e, VC_ESTATE, "no vc_eval_forward call with nll_dev / tgt_dev has run");
    src = e->eval_logits; avail = e->eval_logits_rows * e->K * e->V * 4;
  }
  else if (n == "pe") { src = e->pe; avail = (int64_t)e->S_max * e->d * 4; }
  else if (n == "sampler_ts") { src = e->dbg_ts; avail = 16 * 8; }
  else if (n == "kernel_ts") { src = e->dbg_ts; avail = 64 * 8; }
  else if (n == "host_ms") { host_src = e->host_ms; avail = 8 * 8; }
  else if (n == "options") {        // the option state as text (vc_set_option), NUL-padded
    memset(host_dst, 0, (size_t)nbytes);
    memcpy(host_dst, e->opt_state.c_str(), std::min<size_t>((size_t)nbytes > 0 ? (size_t)nbytes - 1 : 0, e->opt_state.size()));
    return VC_OK;
  }
  else if (std::vector<int32_t> v; pack_stats(e, n, v)) {      // "w13_stats", "w8_stats", "w8w_stats", "w8u_stats", "w8ur_stats", "w8q_stats"
    if (nbytes > (int64_t)(v.size() * 4)) return fail(e, VC_ECAP, "debug buffer '%s' holds %lld bytes", n.c_str(), (long long)(v.size() * 4));
    memcpy(host_dst, v.data(), (size_t)nbytes);
    return VC_OK;
  }
  else if (n == "launch_counts") { host_src = vc_launch_counts; avail = VC_LC_N * 8; }     // process-wide census of kernel forms (vc_common.h)
  else if (n == "launch_counts_more") { host_src = vc_launch_counts + VC_LC_W8_UP_ROWS; avail = (VC_LC_N - VC_LC_W8_UP_ROWS) * 8; }   // the slots from VC_LC_W8_UP_ROWS on
  else if (n == "launch_counts_more2") { host_src = vc_launch_counts + VC_LC_W8_QKV_ROWS; avail = (VC_LC_N - VC_LC_W8_QKV_ROWS) * 8; }   // the slots from VC_LC_W8_QKV_ROWS on
  else if (n == "stream") {         // the open streaming TTS call: {finished rows the host knows of, frames handed out, loop over}
    if (!e->ts) return fail(e, VC_ESTATE, "no streaming TTS call is open (vc_tts_stream_begin)");
    if (nbytes != 3 * 4) return fail(e, VC_ECAP, "debug buffer 'stream' holds 12 bytes");
    const int32_t v[3] = {1 + e->ts->L.complete, e->ts->emitted, e->ts->L.over ? 1 : 0};
    memcpy(host_dst, v, sizeof v);
    return VC_OK;
  }
  else if (n == "session_slots") {  // the open decode session's bookkeeping: {rows of the step in force, ticket holding slot 0, 1, ... (-1 = free)}
    std::vector<int32_t> v;
    if (const int rc = debug_session_slots(e, v)) return rc;
    if (nbytes != (int64_t)(v.size() * 4)) return fail(e, VC_ECAP, "debug buffer 'session_slots' holds %lld bytes", (long long)(v.size() * 4));
    memcpy(host_dst, v.data(), (size_t)nbytes);
    return VC_OK;
  }
  else return fail(e, VC_EINVAL, "unknown debug buffer '%s'", n.c_str());
  if (nbytes > avail) return fail(e, VC_ECAP, "debug buffer '%s' holds %lld bytes", n.c_str(), (long long)avail);
  if (host_src) { memcpy(host_dst, host_src, (size_t)nbytes); return VC_OK; }
  HIPCHK(e, hipDeviceSynchronize());
  HIPCHK(e, hipMemcpy(host_dst, src, (size_t)nbytes, hipMemcpyDeviceToHost));
  return VC_OK;
}

extern "C" int vc_last_timing(const vc_engine* e, float ms[3]) {
  if (!e || !ms) return VC_EINVAL;
  ms[0] = e->ms[0]; ms[1] = e->ms[1]; ms[2] = e->ms[2];
  return VC_OK;
}

// Times one launch site of a pass in isolation (HIP events on the launch stream), on the weights of layer (i % L) (layer 0: _hot).
//   which = "ffn1" | "ffn2" | "qkv" | "oproj" | "attn" : a step of n_rows <= 16 rows; "wd_*" (also "wd_ln"): 17..64 rows; "pf_*": a prefill pass
//   which = "step" : one whole decode step (forward + heads, sampler excluded) for n_rows sequences
extern "C" int vc_bench_kernel(vc_engine* e, const char* which, int n_rows, int iters, float* avg_ms,
                               double* alg_bytes, void* stream) {
  int rc = check_idle(e);
  if (rc) return rc;
  if (!which || n_rows < 1 || iters < 1 || !avg_ms) return fail(e, VC_EINVAL, "bad argument to vc_bench_kernel");
  const bool pf = std::string(which).rfind("pf_", 0) == 0;      // prefill block GEMM: up to VC_MAX_ROWS rows
  const bool wide = std::string(which).rfind("wd_", 0) == 0;    // a linear layer of a wide decode step: 17..VC_MAX_SEQS rows
  if (wide && n_rows <= VC_ROWS) return fail(e, VC_EINVAL, "vc_bench_kernel: '%s' takes 17..%d rows", which, VC_MAX_SEQS);
  if (n_rows > (pf ? VC_MAX_ROWS : wide ? VC_MAX_SEQS : VC_ROWS)) return fail(e, VC_EINVAL, "vc_bench_kernel: %d rows exceed %d", n_rows, pf ? VC_MAX_ROWS : wide ? VC_MAX_SEQS : VC_ROWS);
  if (pf && (n_rows > e->emb_cap || ((std::string(which) == "pf_attn" || std::string(which) == "pf_qkv") && n_rows > e->S_max)))
    return fail(e, VC_EINVAL, "vc_bench_kernel: %d rows exceed the prefill arena / cache", n_rows);
  hipStream_t s = stream ? (hipStream_t)stream : e->own_stream;
  const std::string w = which;
  const int d = e->d;
  // neutral rows: sequence 0, positions 0..n_rows-1 (position only matters to attention/caches)
  std::vector<int> seq(VC_MAX_SEQS, 0), pos(VC_MAX_SEQS, 0);
  for (int i = 0; i < VC_MAX_SEQS; ++i) pos[i] = i;
  if (std::string(which).rfind("attn", 0) == 0)          // attention: a 16 s utterance's worth of cached positions
    for (int i = 0; i < VC_ROWS; ++i) pos[i] = std::min(e->S_max - 1, 883);
  if (pf) {   // prefill row tables: sequence 0, positions 0..n_rows-1
    std::vector<int> pseq(n_rows, 0), ppos(n_rows);
    for (int i = 0; i < n_rows; ++i) ppos[i] = i;
    HIPCHK(e, hipMemcpyAsync(e->pre_row_seq, pseq.data(), (size_t)n_rows * 4, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(e->pre_row_pos, ppos.data(), (size_t)n_rows * 4, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipStreamSynchronize(s));                   // the staging vectors die with this scope
  }
  if (w == "wd_attn")      // every row its own sequence slot, at the last position of a 16 s utterance: n_rows caches streamed
    for (int i = 0; i < VC_MAX_SEQS; ++i) { seq[i] = i % std::max(1, e->B_max); pos[i] = std::min(e->S_max - 1, 883); }
  const int n_tab = wide ? std::min(e->NS, VC_MAX_SEQS) : VC_ROWS;      // (wide: rows 0..n_rows-1 of sequence 0, positions 0.. - needs max_positions >= n_rows)
  if (wide && (n_rows > e->NS || n_rows > e->S_max || n_rows > e->B_max)) return fail(e, VC_EINVAL, "vc_bench_kernel: %d rows exceed max_seqs / max_positions", n_rows);
  HIPCHK(e, hipMemcpyAsync(e->dec_row_seq, seq.data(), (size_t)n_tab * 4, hipMemcpyHostToDevice, s));
  HIPCHK(e, hipMemcpyAsync(e->dec_row_pos, pos.data(), (size_t)n_tab * 4, hipMemcpyHostToDevice, s));
  if (wide) {
    HIPCHK(e, hipMemsetAsync(e->act, 0, (size_t)n_rows * 4 * d * e->esz, s));
    HIPCHK(e, hipMemsetAsync(e->xn, 0, (size_t)n_rows * d * e->esz, s));
  }
  HIPCHK(e, hipMemsetAsync(e->dec_h, 0, (size_t)VC_ROWS * d * 4, s));
  HIPCHK(e, hipMemsetAsync(e->hA, 0, (size_t)VC_ROWS * d * 4, s));
  HIPCHK(e, hipMemsetAsync(e->hB, 0, (size_t)VC_ROWS * d * 4, s));
  HIPCHK(e, hipMemsetAsync(e->parts, 0, (size_t)VC_MAX_KSPLIT * VC_SLAB_ROWS * d * 4, s));
  HIPCHK(e, hipMemsetAsync(e->act, 0, (size_t)VC_ROWS * 4 * d * e->esz, s));
  HIPCHK(e, hipMemsetAsync(e->xn, 0, (size_t)VC_ROWS * d * e->esz, s));
  HIPCHK(e, hipMemsetAsync(e->att_o, 0, (size_t)VC_ROWS * e->H * VC_MAX_NSPLIT * e->hd * 4, s));
  HIPCHK(e, hipMemsetAsync(e->att_ml, 0, (size_t)VC_ROWS * e->H * VC_MAX_NSPLIT * 2 * 4, s));
  HIPCHK(e, hipMemsetAsync(e->logit_row, 0, VC_ROWS * 4, s));
  bool hot = false;
  std::string w2 = w;
  if (w.size() > 4 && w.substr(w.size() - 4) == "_hot") { hot = true; w2 = w.substr(0, w.size() - 4); }
  // the paired launches of 2..8 finished rows by their kernels' names: the sites, refused where the plan does not take the form
  const bool by_frp = w2 == "rows_gemm_frp", by_qp = w2 == "rows_gemm_qp";
  if (by_frp) w2 = "ffn2";
  if (by_qp) w2 = "qkv";
  // The launch site a name times, in the form a pass of n_rows rows launches it at a layer > 0 (wd_*: a 17..64-row decode step; pf_*: a
  // prefill pass, the attention kernel a prompt of n_rows rows gets).  The LayerNorm launch in front of a GEMM is a site of its own.
  const std::string site = (wide || pf) ? w2.substr(3) : w2;
  const bool known = wide ? (site == "ffn1" || site == "ffn2" || site == "oproj" || site == "qkv" || site == "ln" || site == "attn")
                     : pf ? (site == "ffn1" || site == "qkv" || site == "attn")
                          : (site == "ffn1" || site == "ffn2" || site == "oproj" || site == "qkv" || site == "attn" || site == "step");
  if (!known) return fail(e, VC_EINVAL, "unknown kernel '%s'", which);
  const PassPlan p = plan_pass(e, n_rows, wide, pf ? prefill_tiled(e, n_rows) : 0);
  if ((by_frp && !p.frp) || (by_qp && !p.qp)) return fail(e, VC_EINVAL, "vc_bench_kernel: a step of %d rows does not launch '%s' on this engine", n_rows, which);
  RowSrc rs{};
  rs.h_in = e->dec_h; rs.row_seq = pf ? e->pre_row_seq : e->dec_row_seq; rs.row_pos = pf ? e->pre_row_pos : e->dec_row_pos;
  rs.n_rows = n_rows; rs.n_active = wide ? e->one : nullptr; rs.nt = 1;
  rs.rps = pf ? 0 : 1;      // decode sites: a kv8 engine's attention on the E4M3 cache, as its steps launch it
  auto one = [&](int i) -> int {
    const Layer& ly = e->layers[hot ? 0 : i % e->L];   // _hot: the same 8-34 MB every launch (cache-resident)
    const Resid rq = qkv_in(e, p, ly, e->hB, &ly), rf = ffn_in(e, p, ly, e->hB);
    if (site == "qkv") return site_qkv(e, p, rs, ly, rq, &ly, s);
    if (site == "attn") return site_attn(e, p, rs, ly, s);
    if (site == "oproj") return site_oproj(e, p, rs, ly, e->hB, s);
    if (site == "ln") return site_ln(e, rs, rf, s);         // the per-row LayerNorm launch in front of the FFN up-projection
    if (site == "ffn2") return site_ffn_down(e, p, rs, ly, s);
    if (site == "ffn1") {
      const char* dbg_env = pf ? getenv("VC_BLK_DBG") : nullptr;        // tools/blk_probe.py: wrong results by design, timing only
      if (pf) vc_blk_dbg_mask = dbg_env ? atoi(dbg_env) : 0;
      const int r = site_ffn_up(e, p, rs, ly, rf, s);
      if (pf) vc_blk_dbg_mask = 0;
      return r;
    }
    PassOut po;                                              // "step": forward + heads, sampler excluded
    const int r = run_pass(e, p, rs, &po, s);
    return r ? r : run_heads(e, p, po, nullptr, n_rows, 0, 0, nullptr, s);
  };
  for (int i = 0; i < 3; ++i) { rc = one(i); if (rc) return rc; }
  HIPCHK(e, hipEventRecord(e->ev[0], s));
  for (int i = 0; i < iters; ++i) { rc = one(i); if (rc) return rc; }
  HIPCHK(e, hipEventRecord(e->ev[1], s));
  HIPCHK(e, hipStreamSynchronize(s));
  float ms = 0;
  HIPCHK(e, hipEventElapsedTime(&ms, e->ev[0], e->ev[1]));
  *avg_ms = ms / (float)iters;
  if (alg_bytes) {
    const double es = e->esz;
    const double kvb = e->kv8 ? 1.0 + 2.0 / e->hd : es;      // bytes per cached value the decode attention streams (option "kv8": a code byte + the row's share of two shift bytes)
    const std::string& w = w2;
    double b = 0;
    if (w == "wd_ffn1") b = 4.0 * d * d * es + n_rows * (d * es + 4.0 * d * es);
    else if (w == "wd_ffn2") b = 4.0 * d * d * es + n_rows * (4.0 * d * es + d * 4.0 * p.ks_f2);
    else if (w == "wd_qkv") b = 3.0 * d * d * es + n_rows * (d * es + d * 4.0 + 2.0 * d * es);
    else if (w == "wd_oproj") b = 1.0 * d * d * es + n_rows * (d * es + d * 4.0 * p.ks_o);
    else if (w == "wd_ln") b = n_rows * (d * 4.0 * (2 + p.ks_o) + d * es);
    else if (w == "wd_attn") b = n_rows * 2.0 * d * kvb * (std::min(e->S_max - 1, 883) + 1);
    else if (w == "ffn1") b = 4.0 * d * d * es + n_rows * (d * 4.0 + 4.0 * d * es);
    else if (w == "ffn2") b = 4.0 * d * d * es + n_rows * (4.0 * d * es + d * 4.0);
    else if (w == "qkv") b = 3.0 * d * d * es + n_rows * (d * 4.0 + 3.0 * d * es);
    else if (w == "oproj") b = 1.0 * d * d * es + n_rows * (d * 4.0 * 2);
    else if (w == "attn") b = n_rows * 2.0 * d * kvb * (std::min(e->S_max - 1, 883) + 1);   // K and V of every cached position
    else if (w == "pf_qkv") b = 2.0 * n_rows * (double)d * 3.0 * d;                        // FLOPs
    else if (w == "pf_ffn1") b = 2.0 * n_rows * (double)d * 4.0 * d;                       // FLOPs, not bytes (MFMA roofline)
    else if (w == "pf_attn") b = 4.0 * d * ((double)n_rows * (n_rows + 1) / 2.0);          // FLOPs of Q K^T and P V under the causal mask
    else b = (double)e->L * (12.0 * d * d + 13.0 * d) * es + 2.0 * d * es +
             (double)e->K * ((double)d * e->P + e->P + (double)e->P * e->V + e->V) * es;
    *alg_bytes = b;
  }
  return VC_OK;
}
