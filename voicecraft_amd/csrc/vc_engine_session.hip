// vc_engine_session.hip - host side of libvcengine.so: decode sessions (continuous batching).  The session's bookkeeping, the
// steps of a turn, and every vc_session_* entry point.
#include "vc_engine_host.h"

// ------------------------------------------------------------------------------------- decode sessions (continuous batching)
// A session keeps the decode loop open and takes TTS and editing requests at any time (vc_session_submit / _submit_ctl / _submit_edit).
// One TURN (vc_session_advance) is one iteration of DecodeLoop::advance with the way in added:
//   1. wait for the older of the two graph batches in flight;
//   2. count the retirements stamped with a batch the host has now seen END (the sampler writes one pinned record per slot, stamped
//      with the batch index session_turn_k laid down in front of that batch);
//   3. admit from the FIFO into the free slots, in order, as many as fit;
//   4. queue, on the decode stream: the prompts and ONE prefill of the admitted requests into their K/V slots, session_turn_k (stamp of the
//      next batch; re-pack of the live rows onto the width now needed, narrower or wider; the admitted requests' initial states behind
//      them; fillers; n_active raised), the first sample of the admitted rows alone, and the next batch of graph_steps steps.
//      The admitted requests' first states (tts_request for a TTS request; edit_state with feed_switch of an editing request - one row
//      per request, its span switches fed over three steps as in vc_edit_multi) and their sampling controls are written into pinned
//      staging buffer (batch % VC_ADM_STAGES) and uploaded on the decode stream in front of session_turn_k.  That buffer is written again
//      VC_ADM_STAGES turns later at the earliest; a turn queues only after the batch two turns back has ENDED (step 1), and a batch ends
//      behind its turn's upload on the same stream, so no queued upload can still have to read a buffer the host is writing.
// A session opened for best-of-N requests (vc_session_open_best_of, max_samples > 1) takes TTS requests of N samples too
// (vc_session_submit_best_of): one ticket, N rows and N slots.  The prompt is prefilled once, into the first slot, and its K/V copied
// to the siblings' slots (copy_kv_k); the rows are laid next to each other in sample order, with SeqState.group = the ticket and
// their sample index in samp_tab (session_groups_k, behind session_turn_k); the steps of such a session end in the sample / advance
// PAIR (vc_launch_sample_session grouped), whose second launch holds the keep decision.  Every row writes its slot's record, word 6
// = kept: a dropped sample's slot is free once the host has seen its batch end, the request is finished when all N records are in,
// and only the kept sample's slot waits for the fetch.
// What the host decides - who is admitted when, every width - depends only on the submissions, the turn each was made at and records
// of batches that have ended: never on how far the device runs ahead.  The same schedule therefore gives the same tokens in bf16 too.
// Width in force: the next power of two >= live sequences, capped by `top` (that power for max_live where the per-row buffers hold it,
// else max_live itself, as a blocking call of max_live sequences starts at its own count).
struct SessReq {
  int kind = 0;             // 0 TTS (job), 1 editing (edit)
  TtsJob job{};
  EditJob edit{};           // its iv / mv point into iv_own / mv_own (re-pointed wherever a SessReq is copied)
  std::vector<int32_t> iv_own, mv_own;
  vc_request_ctl ctl{};     // the request's sampling controls (the session's when it gave none)
  uint64_t seed = 0;
  int slot = -1;
  int state = 0;            // 0 pending, 1 live, 2 finished
  int total_steps = 0, span = 0, prompt_err = 0, fed = 0;
  int span_steps[VC_MAX_SPANS]{};
  int adm_batch = -1;       // the graph batch queued by the turn that admitted it (vc_session_frames counts its final rows from there)
  int emitted = 0;          // frames vc_session_frames has handed out
  // a best-of-N request (n_samples > 1): one row and one K/V slot per sample.  `slot` is slots[0] while it decodes and the KEPT sample's
  // slot once it has finished (-1 when no sample terminated); total_steps / span / span_steps are then the kept sample's
  int n_samples = 1;
  std::vector<int> slots;   // [n_samples], increasing
  std::vector<char> mdone;  // [n_samples] the member's retirement record has been read
  int members_left = 0;
  int kept = -1;            // sample index of the member that retired kept with its span finished
  // a live request that was cancelled (vc_session_cancel): gone for every entry point, it stays in the table until the records of
  // its rows have been read (session_note_retired), which is what frees its slots
  bool cancelled = false;
  bool cancel_queued = false;   // its rows are in the table of a session_cancel_k launch already queued
};
struct Session {
  DecodeLoop L{};
  hipStream_t s = nullptr;
  vc_sample_cfg sc{};
  int max_live = 0, top = 0;
  int max_samples = 1;      // > 1: opened for best-of-N requests (vc_session_open_best_of) - the steps' sampler is the sample / advance pair
  bool grouped = false;     // max_samples > 1
  int B = 0;                // rows of the step in force (0: nothing laid out yet)
  int live = 0;             // rows (one per sample of a request) admitted and not yet KNOWN to have retired
  int batch = 0;            // index of the next graph batch (never reset: the retirement stamps are unique for the session's life)
  int run_start = 0;        // first batch queued since the session was last idle: only batches from there on can be in flight
  int known = -1;           // the newest batch vc_session_advance has seen END (what vc_session_frames may hand out hangs on this alone)
  int next_ticket = 1;
  std::deque<int> fifo;
  std::map<int, SessReq> reqs;
  std::vector<int> slot_ticket;      // [max_live] ticket holding the slot (live, or finished and not yet fetched), -1 = free
  long long stats[8]{};     // indexed by SS_*
  // decode-stream time of each admission (prefill + session_turn_k + first sample): event pairs, read once their batch has ended
  hipEvent_t ev_adm[4][2]{};
  int ev_turn[4]{-1, -1, -1, -1};
  double adm_ms = 0;
  // a turn whose queued work failed after requests had been admitted on the host: the device and the tables no longer agree, so every
  // later submit / advance / fetch returns this error and the caller closes the session
  bool broken = false;
  std::string broken_msg;
};
namespace {
int session_broken(vc_engine* e, const Session& t) {
  return fail(e, VC_ESTATE, "the decode session failed in an earlier turn (%s): close it (vc_session_close)", t.broken_msg.c_str());
}
}  // namespace
namespace vch __attribute__((visibility("hidden"))) {
void drop_session(vc_engine* e) {
  if (!e->sess) return;
  for (auto& pr : e->sess->ev_adm)
    for (auto& ev : pr) if (ev) (void)hipEventDestroy(ev);
  delete e->sess;
  e->sess = nullptr;
}
}  // namespace vch
namespace {

int session_width(const Session& t, int live) { return std::min(DecodeLoop::width_for(std::max(1, live)), t.top); }

// the admission timings whose batch the host has seen end (all of them when `all`: the stream was synchronised)
void session_read_timers(Session& t, int known, bool all) {
  for (int i = 0; i < 4; ++i) {
    if (t.ev_turn[i] < 0 || (!all && t.ev_turn[i] > known)) continue;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, t.ev_adm[i][0], t.ev_adm[i][1]) == hipSuccess) t.adm_ms += ms;
    t.ev_turn[i] = -1;
  }
}

// retirements stamped with a batch <= known (stamps are batch + 1 in the record)
void session_note_retired(vc_engine* e, Session& t, int known, int* tickets_out, int cap, int* n_fin) {
  for (int slot = 0; slot < t.max_live; ++slot) {
    const int ticket = t.slot_ticket[slot];
    if (ticket < 0) continue;
    SessReq& r = t.reqs[ticket];
    if (r.state != 1) continue;
    volatile int* rec = e->h_rec + slot * VC_SESS_REC;
    const int stamp = rec[0];
    if (stamp == 0 || stamp - 1 > known) continue;
    if (r.cancelled) {
      // a row of a cancelled request, retired by session_cancel_k or - in a batch that was still in flight when the cancel was made - by
      // itself: the slot is free from here on, whatever the record says of `kept`, and nothing is reported (the cancel wins)
      int m = -1;                                       // (a request of one sample has slots = {slot}, as admission laid them)
      for (int i = 0; i < r.n_samples; ++i) if (r.slots[i] == slot) m = i;
      if (m < 0 || r.mdone[m]) continue;
      r.mdone[m] = 1;
      r.members_left -= 1;
      t.live -= 1;
      t.stats[SS_LIVE_ROWS] += std::max(0, (int)rec[1] - 1) + std::max(0, (int)rec[5]);
      t.slot_ticket[slot] = -1;
      if (r.members_left == 0) {
        // (a kept member whose record had been read before the cancel was still holding its slot for the fetch)
        for (int& held : t.slot_ticket) if (held == ticket) held = -1;
        t.reqs.erase(ticket);
      }
      continue;
    }
    if (r.n_samples > 1) {
      // one member of a best-of-N request.  A dropped sample's slot is free from here on; the request is finished - and reported - by
      // the turn that has read all its members' records, and only the kept sample's slot is held for the fetch
      int m = -1;
      for (int i = 0; i < r.n_samples; ++i) if (r.slots[i] == slot) m = i;
      if (m < 0 || r.mdone[m]) continue;
      const bool last = r.members_left == 1;
      if (last && *n_fin >= cap) continue;              // no room to report the request: this member is read again by a later turn
      r.mdone[m] = 1;
      r.members_left -= 1;
      t.live -= 1;
      t.stats[SS_LIVE_ROWS] += std::max(0, (int)rec[1] - 1);
      r.prompt_err |= rec[4];
      if (rec[6] && rec[2] >= 1 && m >= r.kept) {       // (at most one member ends kept with its span finished: advance_phase)
        r.kept = m;
        r.total_steps = rec[1]; r.span = rec[2]; r.fed = rec[5];
        for (int i = 0; i < VC_MAX_SPANS; ++i) r.span_steps[i] = rec[VC_SESS_REC_SPANS + i];
      }
      if (!rec[6]) t.slot_ticket[slot] = -1;
      if (last) {
        r.state = 2;
        for (int i = 0; i < r.n_samples; ++i)
          if (i != r.kept && t.slot_ticket[r.slots[i]] == ticket) t.slot_ticket[r.slots[i]] = -1;
        r.slot = r.kept >= 0 ? r.slots[r.kept] : -1;
        tickets_out[*n_fin] = ticket;
        *n_fin += 1;
      }
      continue;
    }
    if (*n_fin >= cap) continue;                        // no room to report it: it stays live on the host and is reported by a later turn
    r.state = 2;
    r.total_steps = rec[1]; r.span = rec[2]; r.prompt_err = rec[4]; r.fed = rec[5];
    for (int i = 0; i < VC_MAX_SPANS; ++i) r.span_steps[i] = rec[VC_SESS_REC_SPANS + i];
    t.live -= 1;
    // rows of launched steps that were live: every step of the request but its first sample, and the rows an edit fed at its span switches
    t.stats[SS_LIVE_ROWS] += std::max(0, r.total_steps - 1) + std::max(0, r.fed);
    tickets_out[*n_fin] = ticket;
    *n_fin += 1;
  }
}
}  // namespace

extern "C" int vc_session_open_best_of(vc_engine* e, int max_live, int max_samples, const vc_sample_cfg* sc, void* stream) {
  int rc = check_idle(e);
  if (rc) return rc;
  if (!sc) return fail(e, VC_EINVAL, "null argument to vc_session_open");
  if (max_live < 1 || max_live > e->B_max) return fail(e, VC_EINVAL, "vc_session_open: max_live %d outside [1, max_seqs = %d]", max_live, e->B_max);
  if (max_samples < 1 || max_samples > max_live)
    return fail(e, VC_EINVAL, "vc_session_open_best_of: max_samples %d outside [1, max_live = %d]", max_samples, max_live);
  hipStream_t s = stream ? (hipStream_t)stream : e->own_stream;
  Session* t = new Session();
  t->s = s; t->sc = *sc; t->max_live = max_live;
  t->max_samples = max_samples; t->grouped = max_samples > 1;
  t->top = DecodeLoop::width_for(max_live) <= e->NS ? DecodeLoop::width_for(max_live) : max_live;
  t->slot_ticket.assign(max_live, -1);
  auto bail = [&](int code) { e->sess = t; drop_session(e); return code; };
  for (auto& pr : t->ev_adm)
    for (auto& ev : pr)
      if (hipEventCreate(&ev) != hipSuccess) return bail(fail(e, VC_EHIP, "hipEventCreate failed"));
  // silence tokens and the graph switch are the session's (one SampleDyn); the seed and the sampling controls are per request
  // (SampleDyn.seed_tab / ctl_tab by slot), the controls given here being the default of a request that brings none
  if ((rc = push_sample_dyn(e, sc, nullptr, 0, nullptr, 0, max_live, s))) return bail(rc);
  memset(e->h_rec, 0, sizeof(int) * VC_SESS_REC * e->NS);
  e->h_flag[HF_STAGE] = 0; e->h_flag[HF_ACTIVE] = 0; e->h_flag[HF_LIVE0] = 0; e->h_flag[HF_LIVE1] = 0;
  hipError_t he = hipMemsetAsync(e->n_active, 0, sizeof(int), s);
  if (he == hipSuccess) he = hipMemsetAsync(e->step_ctr, 0, sizeof(int), s);
  if (he == hipSuccess) he = hipMemsetAsync(e->batch_id, 0, sizeof(int), s);
  if (he == hipSuccess) he = hipMemsetAsync(e->prompt_err, 0, sizeof(int) * e->NS, s);
  if (he == hipSuccess) he = hipStreamSynchronize(s);       // (orders the reuse of the pinned sampler block, as check_err_flag does in a call)
  if (he != hipSuccess) return bail(fail(e, VC_EHIP, "vc_session_open: %s", hipGetErrorString(he)));
  e->repack_at.clear();
  // every graph the session can pass through, ahead of any timer: the powers of two below `top`, and `top`
  t->L.init(e, make_sample_args(e, t->top, 1), t->top, 1, 0, sc, 0, s);
  t->L.sess = true;
  t->L.grouped = t->grouped;      // graphs of their own: the steps of such a session end in the sample / advance pair
  e->host_ms[HM_CAPTURE] = e->host_ms[HM_INSTANTIATE] = 0;
  if (sc->use_graph) {
    hipGraphExec_t exec = nullptr;
    for (int w = t->top; w >= 1 && rc == VC_OK; w = (w == t->top) ? DecodeLoop::width_for(w) / 2 : w / 2) {
      t->L.B = w; t->L.sa = make_sample_args(e, w, 1);
      rc = t->L.exec_for(&exec);
    }
    if (rc) return bail(rc);
  }
  e->sess = t;
  return VC_OK;
}
extern "C" int vc_session_open(vc_engine* e, int max_live, const vc_sample_cfg* sc, void* stream) {
  return vc_session_open_best_of(e, max_live, 1, sc, stream);
}

namespace {
// the checks every submit starts with; *t_out = the open, unbroken session
int session_for_submit(vc_engine* e, Session** t_out) {
  if (!e) return VC_EINVAL;
  if (!e->sess) return fail(e, VC_ESTATE, "no decode session is open (vc_session_open)");
  if (e->sess->broken) return session_broken(e, *e->sess);
  *t_out = e->sess;
  return VC_OK;
}
// a request's sampling controls: its own, checked, or the session's
int session_ctl(vc_engine* e, const Session& t, const vc_request_ctl* ctl, vc_request_ctl* out) {
  if (!ctl) {
    *out = vc_request_ctl{t.sc.top_k, t.sc.top_p, t.sc.temperature, t.sc.stop_repetition};
    return VC_OK;
  }
  if (!(ctl->temperature > 0.f && ctl->temperature <= 3.0e38f))
    return fail(e, VC_EINVAL, "request controls: temperature %g must be a finite positive number", (double)ctl->temperature);
  if (ctl->top_p != ctl->top_p) return fail(e, VC_EINVAL, "request controls: top_p is not a number");
  *out = *ctl;
  return VC_OK;
}
int session_enqueue(Session& t, SessReq&& r, int* ticket) {
  const int id = t.next_ticket++;
  SessReq& q = t.reqs[id];
  q = std::move(r);
  q.edit.iv = q.iv_own.data(); q.edit.mv = q.mv_own.data();
  t.fifo.push_back(id);
  *ticket = id;
  return VC_OK;
}
}  // namespace

extern "C" int vc_session_submit_ctl(vc_engine* e, const int64_t* x_dev, int Lx, const int64_t* y_dev, int T,
                                     const vc_request_ctl* ctl, uint64_t seed, int* ticket) {
  Session* tp = nullptr;
  if (int rc = session_for_submit(e, &tp)) return rc;
  if (!x_dev || (!y_dev && T > 0) || !ticket) return fail(e, VC_EINVAL, "null/invalid argument to vc_session_submit");
  if (Lx < 1 || T < 0) return fail(e, VC_EINVAL, "empty text or negative prompt length");
  const int n_cols = T + 1;
  if (e->S_max - (Lx + n_cols) - 1 < e->K + 1)
    return fail(e, VC_ECAP, "the prompt alone takes %d of max_positions %d", Lx + n_cols, e->S_max);
  if (((Lx + n_cols + 63) & ~63) > e->emb_cap)
    return fail(e, VC_ECAP, "a prompt of %d rows does not fit the prefill arena of %d rows", Lx + n_cols, e->emb_cap);
  SessReq r;
  if (int rc = session_ctl(e, *tp, ctl, &r.ctl)) return rc;
  r.kind = 0;
  r.job = TtsJob{x_dev, Lx, y_dev, T};
  r.seed = seed;
  return session_enqueue(*tp, std::move(r), ticket);
}

extern "C" int vc_session_submit_best_of(vc_engine* e, const int64_t* x_dev, int Lx, const int64_t* y_dev, int T, int n_samples,
                                         const vc_request_ctl* ctl, uint64_t seed, int* ticket) {
  Session* tp = nullptr;
  if (int rc = session_for_submit(e, &tp)) return rc;
  if (!ticket) return fail(e, VC_EINVAL, "null/invalid argument to vc_session_submit");
  if (n_samples < 1 || n_samples > tp->max_samples)
    return fail(e, VC_EINVAL, "vc_session_submit_best_of: n_samples %d outside [1, max_samples = %d] of this session%s", n_samples,
                tp->max_samples, tp->max_samples == 1 ? " (vc_session_open_best_of opens one for best-of-N requests)" : "");
  int id = 0;
  if (int rc = vc_session_submit_ctl(e, x_dev, Lx, y_dev, T, ctl, seed, &id)) return rc;
  tp->reqs[id].n_samples = n_samples;
  *ticket = id;
  return VC_OK;
}

extern "C" int vc_session_submit(vc_engine* e, const int64_t* x_dev, int Lx, const int64_t* y_dev, int T, uint64_t seed, int* ticket) {
  return vc_session_submit_ctl(e, x_dev, Lx, y_dev, T, nullptr, seed, ticket);
}

extern "C" int vc_session_submit_edit(vc_engine* e, const int64_t* x_dev, int Lx, const int64_t* y_dev, int T,
                                      const int32_t* mask_intervals, int M, const int32_t* mask_values,
                                      const vc_request_ctl* ctl, uint64_t seed, int* ticket) {
  Session* tp = nullptr;
  if (int rc = session_for_submit(e, &tp)) return rc;
  if (!x_dev || !y_dev || !mask_intervals || !mask_values || !ticket) return fail(e, VC_EINVAL, "null argument to vc_session_submit_edit");
  SessReq r;
  if (int rc = session_ctl(e, *tp, ctl, &r.ctl)) return rc;
  r.kind = 1;
  // (edit_prepare refuses a span count outside [1, max_n_spans] before it reads either array: the copies only have to stay inside them)
  const int Mc = std::max(0, std::min(M, VC_MAX_SPANS));
  r.iv_own.assign(mask_intervals, mask_intervals + 2 * (size_t)Mc);
  r.mv_own.assign(mask_values, mask_values + 2 * (size_t)Mc);
  r.edit = EditJob{x_dev, Lx, y_dev, T, r.iv_own.data(), M, r.mv_own.data()};
  if (int rc = edit_prepare(e, r.edit, "")) return rc;
  const int rows = Lx + r.edit.pa.n_cols;
  if (((rows + 63) & ~63) > e->emb_cap)
    return fail(e, VC_ECAP, "a prompt of %d rows does not fit the prefill arena of %d rows", rows, e->emb_cap);
  r.seed = seed;
  return session_enqueue(*tp, std::move(r), ticket);
}

namespace {

// The steps of a turn, in the order vc_session_advance takes them (numbered as in the comment above Session).
// ---- 1, 2: the older batch in flight, and what it (or an earlier one) retired
int turn_retire(vc_engine* e, Session& t, int* tickets_out, int cap, int* n_finished) {
  int known = t.run_start - 1;
  if (t.batch - t.run_start >= 2) {
    HIPCHK(e, hipEventSynchronize(e->ev_pace[t.batch & 1]));
    known = t.batch - 2;
  }
  t.known = std::max(t.known, known);
  session_note_retired(e, t, known, tickets_out, cap, n_finished);
  session_read_timers(t, known, false);
  return VC_OK;
}

// ---- the cancels made since the last turn: the slots of the cancelled tickets' rows whose records are still out, one table for
// session_cancel_k (queued in step 4, in front of session_turn_k).  Their slots stay taken until those records have been read
void turn_cancels(Session& t, SessCancelArgs& ca) {
  memset(&ca, 0, sizeof ca);
  for (int slot = 0; slot < t.max_live; ++slot) {
    const int ticket = t.slot_ticket[slot];
    if (ticket < 0) continue;
    const SessReq& r = t.reqs[ticket];
    if (!r.cancelled || r.cancel_queued) continue;
    int m = -1;
    for (int i = 0; i < r.n_samples; ++i) if (r.slots[i] == slot) m = i;
    if (m >= 0 && !r.mdone[m]) ca.slot[ca.n++] = slot;
  }
  for (auto& kv_req : t.reqs) if (kv_req.second.cancelled) kv_req.second.cancel_queued = true;
}

// What step 3 admits on the host and step 4 queues on the decode stream.
struct Admission {
  SessTurnArgs ta;
  SessGroupArgs ga;
  CopyKvArgs kv;            // the siblings' prompt K/V: one (source, destination) entry per sibling, every group of the turn in one table
  std::vector<PromptArgs> pas;
  std::vector<int> slots;
  int n_req = 0;
  SeqState* h_adm_st = nullptr;           // this turn's staging buffers (set by turn_admit)
  vc_request_ctl* h_adm_ctl = nullptr;
};

// ---- 3: admission, FIFO, as many as have a free slot
void turn_admit(vc_engine* e, Session& t, Admission& a) {
  SessTurnArgs& ta = a.ta;
  SessGroupArgs& ga = a.ga;
  CopyKvArgs& kv = a.kv;
  memset(&ta, 0, sizeof ta);
  // this turn's staging buffers (see the comment above Session: the host last wrote them VC_ADM_STAGES turns ago)
  SeqState* const h_adm_st = a.h_adm_st = e->h_adm_st + (size_t)(t.batch % VC_ADM_STAGES) * e->NS;
  vc_request_ctl* const h_adm_ctl = a.h_adm_ctl = e->h_adm_ctl + (size_t)(t.batch % VC_ADM_STAGES) * e->NS;
  // strictly FIFO: the head of the queue is admitted by the first turn that has a free slot for EACH of its samples - the lowest free
  // slots, which need not be consecutive -, and nothing behind it overtakes it (a best-of-N request waiting for slots blocks the line).
  // A request of one sample takes the lowest free slot, as ever.
  memset(&ga, 0, sizeof ga);
  memset(&kv, 0, sizeof kv);
  while (!t.fifo.empty()) {
    const int id = t.fifo.front();
    SessReq& r = t.reqs[id];
    const int N = r.n_samples;
    std::vector<int> mine;
    for (int slot = 0; slot < t.max_live && (int)mine.size() < N; ++slot)
      if (t.slot_ticket[slot] < 0) mine.push_back(slot);
    if ((int)mine.size() < N) break;
    t.fifo.pop_front();
    a.n_req += 1;
    r.slot = mine[0]; r.state = 1; r.adm_batch = t.batch;
    r.slots = mine; r.mdone.assign(N, 0); r.members_left = N; r.kept = -1;
    // the request's first state and its prompt, by kind: what tts_prepare / vc_edit_multi lay down for a sequence of a blocking call
    SeqState st0;
    PromptArgs pa;
    if (r.kind == 1) {
      st0 = edit_state(e, r.edit);
      st0.feed_switch = 1;
      pa = r.edit.pa;
    } else {
      st0 = tts_request(e, r.job, 0, nullptr, &pa);
    }
    if (N > 1) st0.group = id;                              // the group of the keep decision is the request (advance_phase)
    a.pas.push_back(pa);                                    // ONE prefill per request, into its first slot
    a.slots.push_back(mine[0]);
    for (int m = 0; m < N; ++m) {                           // one row per sample, consecutive and in sample order
      const int slot = mine[m];
      t.slot_ticket[slot] = id;
      const int j = ta.n_new++;
      ta.seed[j] = r.seed;
      h_adm_st[j] = st0;
      h_adm_st[j].slot = slot;
      h_adm_ctl[j] = r.ctl;
      ga.slot[j] = slot; ga.lrow[j] = mine[0]; ga.samp[j] = m | (N << 16);
      if (m > 0) {
        const int k = kv.n_ent++;
        kv.src[k] = mine[0]; kv.dst0[k] = slot; kv.cnt[k] = 1; kv.p0[k] = 0; kv.p1[k] = r.job.Lx + r.job.T + 1;
      }
      volatile int* rec = e->h_rec + slot * VC_SESS_REC;    // the slot's record: empty until its row retires
      for (int i = 0; i < VC_SESS_REC; ++i) rec[i] = 0;
    }
  }
}

// nothing to decode: what is still queued is steps without a live sequence.  Wait for them and queue nothing more; a later
// submit (or the fetch that frees a slot for a pending request) restarts the loop.
int turn_idle(vc_engine* e, Session& t, int* tickets_out, int cap, int* n_finished, int* idle) {
  hipStream_t s = t.s;
  if (t.batch > t.run_start) {
    HIPCHK(e, hipStreamSynchronize(s));
    t.known = t.batch - 1;
    session_note_retired(e, t, t.batch - 1, tickets_out, cap, n_finished);
    session_read_timers(t, t.batch - 1, true);
    t.run_start = t.batch;
    if (int rc = check_err_flag(e, s)) return rc;        // (session_turn_k's row check; the stream is idle, so this costs nothing)
  }
  *idle = t.fifo.empty() ? 1 : 0;
  return VC_OK;
}

// ---- 4: prefill of the admitted requests, the turn kernel, their first sample, the next batch
int turn_queue(vc_engine* e, Session& t, Admission& a, SessCancelArgs& ca) {
  SessTurnArgs& ta = a.ta;
  SessGroupArgs& ga = a.ga;
  CopyKvArgs& kv = a.kv;
  hipStream_t s = t.s;
  const int G = t.L.G;
  const int n_new = ta.n_new;                               // ROWS admitted this turn
  const int live_before = t.live;
  const int w = session_width(t, t.live + n_new);
  const int ei = t.batch & 3;
  if (n_new > 0) {
    HIPCHK(e, hipEventRecord(t.ev_adm[ei][0], s));
    int rc = prefill_batch(e, a.pas, a.slots, s, true);
    if (rc) return rc;
    if (kv.n_ent > 0) {
      // prefill once, replicate: prompt positions [0, Lx + T + 1) of each group's first slot to its siblings' slots, one launch per
      // cache tensor for every group of the turn.  The first-step logits are not copied: every member's first sample reads the row
      // of the group's first slot (session_groups_k)
      kv.n_dst = kv.n_ent;
      if ((rc = replicate_kv(e, kv, s))) return rc;
    }
    HIPCHK(e, hipMemcpyAsync(e->adm_st, a.h_adm_st, sizeof(SeqState) * n_new, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(e->adm_ctl, a.h_adm_ctl, sizeof(vc_request_ctl) * n_new, hipMemcpyHostToDevice, s));
  }
  ta.st = e->st; ta.dec_h = e->dec_h; ta.row_seq = e->dec_row_seq; ta.row_pos = e->dec_row_pos; ta.logit_row = e->logit_row;
  ta.err = e->err_flag; ta.n_active = e->n_active; ta.batch_id = e->batch_id; ta.row_base = e->row_base; ta.adm_slot = e->adm_slot;
  ta.seed_tab = e->seed_tab; ta.prompt_err = e->prompt_err; ta.retire_rec = e->h_rec;
  ta.ctl_tab = e->ctl_tab; ta.adm_st = e->adm_st; ta.adm_ctl = e->adm_ctl;
  ta.B_old = t.B; ta.B_new = w; ta.d = e->d; ta.batch = t.batch; ta.repack = (n_new > 0 || w != t.B) ? 1 : 0;
  if (ca.n > 0 && t.B > 0) {
    // (stamped with the batch queued below, not the one in flight: that batch's pacing event was recorded before this launch)
    ca.st = e->st; ca.row_pos = e->dec_row_pos; ca.n_active = e->n_active; ca.retire_rec = e->h_rec; ca.B = t.B; ca.batch = t.batch;
    HIPCHK(e, vc_launch_session_cancel(ca, e->NS, s));
  }
  HIPCHK(e, vc_launch_session_turn(ta, s));
  if (t.grouped && n_new > 0) {
    ga.adm_slot = e->adm_slot; ga.samp_tab = e->samp_tab; ga.n_new = n_new;
    HIPCHK(e, vc_launch_session_groups(ga, e->NS, s));
  }
  if (t.B > 0 && w > t.B) t.stats[SS_WIDENINGS] += 1;
  if (w < t.B) t.stats[SS_NARROWINGS] += 1;
  t.B = w;
  t.L.B = w; t.L.sa = make_sample_args(e, w, 1);
  if (n_new > 0) {
    HIPCHK(e, vc_launch_sample_session(t.L.sa, true, n_new, t.grouped, s));
    HIPCHK(e, hipEventRecord(t.ev_adm[ei][1], s));
    t.ev_turn[ei] = t.batch;
    t.stats[SS_ADMITTED] += a.n_req;                                   // requests; the row sums SS_LIVE_ROWS, SS_LAUNCHED_ROWS count every sample's rows
    if (live_before > 0) t.stats[SS_ADMITTED_LIVE] += a.n_req;
    t.live += n_new;
  }
  if (const int rc = t.L.queue_batch(t.batch & 1)) return rc;
  t.batch += 1;
  t.stats[SS_LAUNCHED_ROWS] += (long long)w * G;
  return VC_OK;
}

}  // namespace

extern "C" int vc_session_advance(vc_engine* e, int* tickets_out, int cap, int* n_finished, int* idle) {
  if (!e) return VC_EINVAL;
  if (!e->sess) return fail(e, VC_ESTATE, "no decode session is open (vc_session_open)");
  if (!n_finished || !idle || cap < 0 || (cap > 0 && !tickets_out)) return fail(e, VC_EINVAL, "null/invalid argument to vc_session_advance");
  HIPCHK(e, hipSetDevice(e->device));
  Session& t = *e->sess;
  if (t.broken) return session_broken(e, t);
  *n_finished = 0; *idle = 0;
  t.stats[SS_TURNS] += 1;
  if (const int rc = turn_retire(e, t, tickets_out, cap, n_finished)) return rc;
  SessCancelArgs ca;
  turn_cancels(t, ca);
  Admission a;
  turn_admit(e, t, a);
  if (t.live + a.ta.n_new == 0) return turn_idle(e, t, tickets_out, cap, n_finished, idle);
  // the requests are admitted on the host already: if anything of the queued work fails the session is marked broken (see Session.broken)
  const int rc4 = turn_queue(e, t, a, ca);
  if (rc4) { t.broken = true; t.broken_msg = e->err; }
  return rc4;
}

extern "C" int vc_session_fetch(vc_engine* e, int ticket, int64_t* res_dev, int res_cap, int* gen_len, int* n_steps) {
  if (!e) return VC_EINVAL;
  if (!e->sess) return fail(e, VC_ESTATE, "no decode session is open (vc_session_open)");
  Session& t = *e->sess;
  auto it = t.reqs.find(ticket);
  if (it == t.reqs.end() || it->second.cancelled)
    return fail(e, VC_EINVAL, "vc_session_fetch: unknown ticket %d (never issued, or fetched or cancelled already)", ticket);
  if (it->second.state != 2) {
    if (t.broken) return session_broken(e, t);
    return fail(e, VC_ESTATE, "vc_session_fetch: the request of ticket %d has not finished", ticket);
  }
  HIPCHK(e, hipSetDevice(e->device));
  SessReq r = std::move(it->second);
  r.edit.iv = r.iv_own.data(); r.edit.mv = r.mv_own.data();
  // whatever the outcome the ticket is spent: the slot (its K/V rows, its rows of the generated-token log) is free for the next request
  // (of a best-of-N request only the kept sample's slot is still held, and none when no sample terminated)
  if (r.slot >= 0) t.slot_ticket[r.slot] = -1;
  t.reqs.erase(it);
  if (!res_dev) return VC_OK;                               // dropped
  if (!gen_len || res_cap < 0) return fail(e, VC_EINVAL, "null/invalid argument to vc_session_fetch");
  if (r.prompt_err & 1)
    return fail(e, VC_EINVAL, "ticket %d: token id out of range in x or y (text rows %d, audio vocab %d)", ticket, e->cfg.text_rows, e->V);
  if (r.n_samples > 1 && r.kept < 0)
    return fail(e, VC_ECAP, "ticket %d: no sample terminated within the step budget", ticket);
  SeqState st;              // what the assembly reads of the request's final state, from the slot's record
  memset(&st, 0, sizeof st);
  st.done = 1; st.span = r.span; st.total_steps = r.total_steps;
  for (int i = 0; i < VC_MAX_SPANS; ++i) st.span_steps[i] = r.span_steps[i];
  // on the side stream: the request's rows of the log are final (its batch has ended), and the decode stream's queued batches are not waited for
  int rc;
  if (r.kind == 1) {
    char who[32];
    snprintf(who, sizeof who, "ticket %d: ", ticket);
    rc = edit_assemble(e, r.edit, st, e->gen + (size_t)r.slot * e->gen_cap * e->K, res_dev, res_cap, gen_len, e->side_stream, who);
  } else {
    rc = assemble_tts(e, r.job, r.slot, st, res_dev, res_cap, gen_len, e->side_stream);
  }
  if (rc) return rc;
  HIPCHK(e, hipStreamSynchronize(e->side_stream));
  if (n_steps) *n_steps = r.total_steps;
  return VC_OK;
}

extern "C" int vc_session_kept(vc_engine* e, int ticket, int* kept) {
  if (!e) return VC_EINVAL;
  if (!e->sess) return fail(e, VC_ESTATE, "no decode session is open (vc_session_open)");
  if (!kept) return fail(e, VC_EINVAL, "null argument to vc_session_kept");
  Session& t = *e->sess;
  auto it = t.reqs.find(ticket);
  if (it == t.reqs.end() || it->second.cancelled)
    return fail(e, VC_EINVAL, "vc_session_kept: unknown ticket %d (never issued, or fetched or cancelled already)", ticket);
  if (it->second.state != 2) {
    if (t.broken) return session_broken(e, t);
    return fail(e, VC_ESTATE, "vc_session_kept: the request of ticket %d has not finished", ticket);
  }
  *kept = it->second.n_samples > 1 ? it->second.kept : 0;   // (-1: no sample of the group terminated - the fetch returns VC_ECAP)
  return VC_OK;
}

// Cancels a request in whatever state it is in (*was: 0 pending, 1 live, 2 finished and not yet fetched).  Host bookkeeping only: the
// call waits for nothing and queues nothing - the rows of a live ticket are retired by session_cancel_k in the next vc_session_advance.
extern "C" int vc_session_cancel(vc_engine* e, int ticket, int* was) {
  if (!e) return VC_EINVAL;
  if (!e->sess) return fail(e, VC_ESTATE, "no decode session is open (vc_session_open)");
  Session& t = *e->sess;
  if (t.broken) return session_broken(e, t);
  auto it = t.reqs.find(ticket);
  if (it == t.reqs.end() || it->second.cancelled)
    return fail(e, VC_EINVAL, "vc_session_cancel: unknown ticket %d (never issued, or fetched or cancelled already)", ticket);
  SessReq& r = it->second;
  int state = r.state;
  if (state == 1) {
    // live on the host - but finished as far as the host can know, if the records of all its rows are stamped with batches advance has
    // seen end (a turn whose tickets_out was full leaves such a request unreported): then it is a finished ticket
    bool all_in = true;
    for (int i = 0; i < r.n_samples && all_in; ++i) {
      if (r.mdone[i]) continue;
      volatile int* rec = e->h_rec + r.slots[i] * VC_SESS_REC;
      const int stamp = rec[0];
      all_in = stamp != 0 && stamp - 1 <= t.known;
    }
    if (all_in) {
      for (int i = 0; i < r.n_samples; ++i) {
        if (r.mdone[i]) continue;
        volatile int* rec = e->h_rec + r.slots[i] * VC_SESS_REC;
        t.live -= 1;
        t.stats[SS_LIVE_ROWS] += std::max(0, (int)rec[1] - 1) + std::max(0, (int)rec[5]);
      }
      for (int& held : t.slot_ticket) if (held == ticket) held = -1;
      r.slot = -1;
      state = 2;
    }
  }
  if (state == 0) {
    // pending: out of the line, the order of the others unchanged; its prompt is never read
    for (auto f = t.fifo.begin(); f != t.fifo.end(); ++f)
      if (*f == ticket) { t.fifo.erase(f); break; }
    t.reqs.erase(it);
  } else if (state == 2) {
    // finished and not fetched: vc_session_fetch(res_dev = NULL)
    if (r.slot >= 0) t.slot_ticket[r.slot] = -1;
    t.reqs.erase(it);
  } else {
    // live: every row of it that has not retired is retired by the next turn, and the slots come back when the host has read their
    // records (session_note_retired) - the path of any retirement, so the schedule stays a function of the calls alone
    r.cancelled = true;
    r.cancel_queued = false;
  }
  if (was) *was = state;
  return VC_OK;
}

namespace {
// Frames of a TTS request the host knows to be final, from the submission schedule alone: the batches vc_session_advance has seen end
// (t.known) and the slot's retirement record once its batch is among them - whether or not the retirement has been reported yet
// (session_note_retired leaves a request live when tickets_out is full).  *ended: the count is the request's last.
int session_final_frames(vc_engine* e, const Session& t, const SessReq& r, bool* ended) {
  *ended = false;
  if (r.state == 0 || r.adm_batch < 0 || t.known < r.adm_batch) return 0;
  int spans = 0, s0 = 0, perr = 0;
  if (r.state == 2) {
    *ended = true; spans = r.span; s0 = r.span_steps[0]; perr = r.prompt_err;
  } else {
    volatile int* rec = e->h_rec + r.slot * VC_SESS_REC;
    const int stamp = rec[0];
    perr = rec[4];                                           // (written by the admitting turn's kernel, in front of batch adm_batch)
    if (stamp != 0 && stamp - 1 <= t.known) { *ended = true; spans = rec[2]; s0 = rec[3]; }
  }
  if (perr & 1) return 0;                                    // an out-of-range token id in the prompt: nothing of it is handed out
  if (*ended) return spans >= 1 ? std::max(0, s0 - e->K) : 0;      // (ran out of positions: no result, no further frames)
  const long rows = 1 + (long)t.L.G * (t.known - r.adm_batch + 1);  // its first sample + graph_steps steps per ended batch
  return (int)std::max(0L, std::min(rows, (long)e->gen_cap) - (e->K - 1));
}
}  // namespace

namespace vch __attribute__((visibility("hidden"))) {
// vc_debug_read "session_slots": {rows of the step in force, ticket holding slot 0, 1, ... (-1 = free)} of the open decode session
int debug_session_slots(vc_engine* e, std::vector<int32_t>& out) {
  if (!e->sess) return fail(e, VC_ESTATE, "no decode session is open (vc_session_open)");
  std::vector<int32_t> v{e->sess->B};
  v.insert(v.end(), e->sess->slot_ticket.begin(), e->sess->slot_ticket.end());
  out.swap(v);
  return VC_OK;
}
}  // namespace vch

extern "C" int vc_session_frames(vc_engine* e, int n, const int* tickets, int min_frames, int64_t* codes_dev, int cap,
                                 int* first_frame, int* n_frames, int* done) {
  if (!e) return VC_EINVAL;
  if (!e->sess) return fail(e, VC_ESTATE, "no decode session is open (vc_session_open)");
  Session& t = *e->sess;
  if (t.broken) return session_broken(e, t);
  if (!tickets || !codes_dev || !first_frame || !n_frames || !done) return fail(e, VC_EINVAL, "null argument to vc_session_frames");
  if (n < 1 || n > t.max_live) return fail(e, VC_EINVAL, "vc_session_frames: %d tickets outside [1, max_live = %d]", n, t.max_live);
  if (cap < 1 || min_frames < 1 || min_frames > cap)
    return fail(e, VC_EINVAL, "vc_session_frames: min_frames %d outside [1, cap = %d]", min_frames, cap);
  // every refusal before any cursor moves
  for (int i = 0; i < n; ++i) {
    auto it = t.reqs.find(tickets[i]);
    if (it == t.reqs.end() || it->second.cancelled)
      return fail(e, VC_EINVAL, "vc_session_frames: unknown ticket %d (never issued, or fetched or cancelled already)", tickets[i]);
    if (it->second.kind == 1)
      return fail(e, VC_EINVAL, "vc_session_frames: ticket %d: editing requests do not stream (their rows per batch hang on span "
                  "switches known at retirement only, and their result is a splice)", tickets[i]);
    if (it->second.n_samples > 1)
      return fail(e, VC_EINVAL, "vc_session_frames: ticket %d: best-of-N requests do not stream (the kept sample is unknown until the "
                  "group decides)", tickets[i]);
    for (int k = 0; k < i; ++k)
      if (tickets[k] == tickets[i]) return fail(e, VC_EINVAL, "vc_session_frames: ticket %d given twice", tickets[i]);
  }
  SessionGatherArgs a;
  memset(&a, 0, sizeof a);
  a.gen = e->gen; a.out = codes_dev; a.K = e->K; a.gen_stride = e->gen_cap; a.cap = cap; a.n = n;
  int any = 0;
  for (int i = 0; i < n; ++i) {
    const SessReq& r = t.reqs[tickets[i]];
    bool ended = false;
    const int avail = session_final_frames(e, t, r, &ended) - r.emitted;
    const int cnt = (avail >= min_frames || (ended && avail > 0)) ? std::min(avail, cap) : 0;
    a.slot[i] = std::max(0, r.slot); a.first[i] = r.emitted; a.count[i] = cnt;
    first_frame[i] = r.emitted; n_frames[i] = cnt;
    done[i] = (ended && avail - cnt <= 0) ? 1 : 0;
    any += cnt;
  }
  if (any > 0) {
    // on the side stream, and that stream alone is waited for: the rows read are final, the decode stream's queued batches are not touched
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, vc_launch_session_gather(a, e->side_stream));
    HIPCHK(e, hipStreamSynchronize(e->side_stream));
  }
  for (int i = 0; i < n; ++i) t.reqs[tickets[i]].emitted += n_frames[i];
  return VC_OK;
}

extern "C" int vc_session_stats(vc_engine* e, int64_t out[8]) {
  if (!e) return VC_EINVAL;
  if (!e->sess) return fail(e, VC_ESTATE, "no decode session is open (vc_session_open)");
  if (!out) return fail(e, VC_EINVAL, "null argument to vc_session_stats");
  const Session& t = *e->sess;
  for (int i = 0; i < 7; ++i) out[i] = t.stats[i];
  out[7] = (int64_t)(t.adm_ms * 1000.0);                    // microseconds of decode-stream time spent on admissions whose batch has ended
  return VC_OK;
}

extern "C" int vc_session_close(vc_engine* e) {
  if (!e) return VC_EINVAL;
  if (!e->sess) return fail(e, VC_ESTATE, "no decode session is open (vc_session_open)");
  HIPCHK(e, hipSetDevice(e->device));
  Session& t = *e->sess;
  int rc = VC_OK;
  // wait for what is queued; the next call uploads every state afresh (vc_tts_stream_end with res_dev = NULL is the model)
  hipError_t he = hipMemsetAsync(e->n_active, 0, sizeof(int), t.s);
  if (he == hipSuccess) he = hipStreamSynchronize(t.s);
  if (he != hipSuccess) rc = fail(e, VC_EHIP, "vc_session_close: %s", hipGetErrorString(he));
  else rc = check_err_flag(e, t.s);                         // (reads and clears the flag word)
  e->cur_rows = 0;
  drop_session(e);
  return rc;
}
