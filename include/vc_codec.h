/*
 * vc_codec.h — C ABI of the EnCodec (SEANet + LSTM + RVQ) encode/decode path in libvcengine.so.
 *
 * Replaces AudioTokenizer.encode / .decode of the reference (data/tokenizer.py:127-133), which call
 * audiocraft's EncodecModel (audiocraft @ c5157b5, not vendored in the reference tree).  The
 * architecture restated here is the one `transformers.EncodecModel` implements for the VoiceCraft
 * codec shape: 16 kHz mono, 64 base filters, strides 2/4/5/8 (hop 320, 50 Hz),
 * 1 residual unit per stage, 2-layer LSTM with skip, weight-normalised convolutions, ELU,
 * reflect padding, non-causal, RVQ of n_q x codebook_size x hidden.
 *
 * Conventions are those of vc_engine.h: plain C, opaque handle, device pointers, a hipStream_t as
 * void*, 0 / negative VC_E* return codes with vc_codec_last_error().
 */
#ifndef VC_CODEC_H
#define VC_CODEC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VC_CODEC_MAX_RATIOS 8

typedef struct vc_codec vc_codec;

typedef struct vc_codec_cfg {
  /* Accepted ranges (vc_codec_create refuses everything else with VC_EINVAL and a message naming the field); the value in
   * front is the VoiceCraft codec's.  Tested range: DESIGN.md section 6. */
  int32_t sample_rate;          /* 16000 (informational)                               */
  int32_t n_filters;            /* 64: any positive multiple of 32                     */
  int32_t n_ratios;             /* 4: 1..VC_CODEC_MAX_RATIOS                            */
  int32_t ratios[VC_CODEC_MAX_RATIOS]; /* decoder (upsampling) order: 8,5,4,2; each >= 2 (transposed kernel = 2 * ratio) */
  int32_t hidden;               /* 128: latent / codebook dimension, any positive multiple of 16 (the MFMA search up to 256) */
  int32_t n_q;                  /* 4 quantizers (K): 1..8                              */
  int32_t codebook_size;        /* 2048: >= 1 (the MFMA search needs a multiple of 16, else the scalar search runs) */
  int32_t lstm_layers;          /* 2: >= 1.  Batched calls need 2 layers at an LSTM width (n_filters * 2^n_ratios) that is a
                                 *    multiple of 256 up to 1024; the decode stream carries at most 2 layers       */
  int32_t kernel_size;          /* 7: first conv, >= 1 (even sizes pad one more on the left) */
  int32_t last_kernel_size;     /* 7: >= 1                                             */
  int32_t residual_kernel_size; /* 3: >= 1                                             */
  int32_t compress;             /* 2: residual unit hidden = dim / compress (only 2)   */
  int32_t max_samples;          /* capacity: longest waveform (samples) per encode call, >= 1; a decode call or a stream
                                 *    window takes up to ceil(max_samples / hop) frames                             */
  /* Architecture switches of the SEANet stacks.  Which values the reference's checkpoint
   * (audiocraft encodec_4cb2048_giga.th, data/tokenizer.py:109-110) was trained with cannot be read from the
   * reference tree, so they are configuration, named as in transformers.EncodecConfig: */
  int32_t causal;               /* use_causal_conv: all padding on the left, transposed convs trimmed on the right */
  int32_t pad_reflect;          /* pad_mode: 1 = "reflect", 0 = "constant" (zeros)     */
  int32_t conv_shortcut;        /* use_conv_shortcut: 1x1 conv on the residual path (else identity) */
  int32_t num_residual_layers;  /* residual units per stage (1): 1..4                  */
  int32_t dilation_growth_rate; /* unit j dilates its first conv by rate**j (2): 1..4  */
  int32_t max_batch;            /* capacity: clips per vc_codec_encode_batch / decode_batch call: 1..64 */
} vc_codec_cfg;

int vc_codec_create(const vc_codec_cfg* cfg, int hip_device, vc_codec** out);
void vc_codec_destroy(vc_codec* c);
const char* vc_codec_last_error(const vc_codec* c);

/* Effective fp32 tensors (weight norm already folded: w = g * v / ||v||), keyed like the
 * transformers.EncodecModel modules:
 *   encoder.layers.{i}.conv.{weight,bias}            Conv1d        [Co][Ci][Kw]
 *   encoder.layers.{i}.block.{1,3}.conv.{weight,bias}
 *   {encoder,decoder}.layers.{i}.lstm.{weight_ih,weight_hh,bias_ih,bias_hh}_l{n}
 *   decoder.layers.{i}.conv.{weight,bias}            Conv1d or ConvTranspose1d [Ci][Co][Kw]
 *   quantizer.layers.{q}.codebook.embed              [codebook_size][hidden]               */
int vc_codec_load_tensor(vc_codec* c, const char* key, const void* data, int on_device,
                         const int64_t* shape, int ndim);
int vc_codec_finalize(vc_codec* c);

/* AudioTokenizer.encode (data/tokenizer.py:127-129): wav fp32 [n_samples] -> codes int64 [K][T],
 * T = ceil(n_samples / hop).  *n_frames receives T. */
int vc_codec_encode(vc_codec* c, const float* wav_dev, int n_samples, int64_t* codes_dev,
                    int codes_cap, int* n_frames, void* stream);
/* AudioTokenizer.decode (data/tokenizer.py:131-133): codes int64 [K][T] -> wav fp32 [hop*T]. */
int vc_codec_decode(vc_codec* c, const int64_t* codes_dev, int T, float* wav_dev, int wav_cap,
                    void* stream);
/* Bulk forms: the reference's dataset encoder pushes a zero-padded batch [B,1,N] through ONE model.encode call
 * (data/phonemize_encodec_encode_hf.py:186-206) and AudioTokenizer.encode/decode take [B,...] tensors.
 *   encode_batch: wav fp32 [B][n_samples] (already padded to a common length) -> codes int64 [B][K][T]
 *   decode_batch: codes int64 [B][K][T] -> wav fp32 [B][hop*T]
 * Every item gives bit for bit what the single-clip call gives on the same (padded) row: the batch is an extra
 * grid dimension of the convolutions and the LSTM advances all B sequences per launch (one read of the
 * recurrence weights for the whole batch).  codes_cap / wav_cap are per item. */
int vc_codec_encode_batch(vc_codec* c, const float* wav_dev, int B, int n_samples, int64_t* codes_dev,
                          int codes_cap, int* n_frames, void* stream);
int vc_codec_decode_batch(vc_codec* c, const int64_t* codes_dev, int B, int T, float* wav_dev, int wav_cap,
                          void* stream);
/* ---- chunked decode: the waveform of a code sequence that is still being produced (one clip; vc_codec_decode_streams below
 * advances many).
 * The decoder is an RVQ look-up, one conv over frames, a UNIDIRECTIONAL LSTM and a purely local upsampling stack, so it can
 * run chunk by chunk with the LSTM's (h, c) carried between calls and a few frames of look-ahead - exactly: the
 * concatenation of everything a stream emits is, BIT FOR BIT, what vc_codec_decode gives for the concatenation of
 * everything it was fed, for any split into chunks (chunks of one frame, a total shorter than the look-ahead, an empty
 * final call).  Every frame passes the look-up, the first conv and the LSTM once; the stack behind the LSTM runs over a
 * window = the frames to hand out plus the context frames on either side, and only the interior samples leave.
 *
 *   vc_codec_stream_geometry (host only, no handle, no GPU), all three in frames, derived from the config (kernel
 *   sizes, ratios, num_residual_layers, dilation_growth_rate, causal, pad_reflect):
 *     lookahead_frames     the samples of frame t are final - and emitted - once frame t + lookahead has been fed
 *                          (right context of the first conv + of the stack behind the LSTM; 0 with causal = 1)
 *     left_context_frames  behind the LSTM, the output of frame p reaches no sample of frames >= p + left_context
 *                          (its own frame counts: the window keeps left_context - 1 frames in front of the emitted ones)
 *     start_frames         (may be NULL) nothing is emitted before this many frames have been fed: reflect padding at
 *                          the true start mirrors the frames behind it, and a clip no longer than its padding is
 *                          zero-extended first, so the first conv must know the clip is longer than that.  1 with
 *                          constant padding.
 *   After feeding F frames in all, hop * (F >= start_frames ? max(0, F - lookahead_frames) : 0) samples have been
 *   emitted; the call with last = 1 emits the rest (hop * F in all) and closes the stream.
 *
 *   vc_codec_decode_stream_begin  opens the handle's decode stream (zero LSTM state); a second begin restarts it.
 *                                 A codec with more than 2 LSTM layers has no stream: VC_EINVAL with a message.
 *   vc_codec_decode_stream        codes_dev int64 [K][n] with row stride `stride` (>= n): the next n frames (n = 0 is
 *                                 legal, e.g. a final call that only flushes); wav_dev receives *n_samples_out samples
 *                                 (wav_cap too small: VC_ECAP, nothing consumed).  The call returns with the samples
 *                                 written (it synchronises `stream`): the activation arenas are shared with the
 *                                 blocking calls, so vc_codec_encode / vc_codec_decode between two calls of an open
 *                                 stream are legal and do not disturb it.  What the stream remembers - the (h, c) of
 *                                 both LSTM layers, the latents in front of the first conv, the LSTM outputs the next
 *                                 window needs, the frame counters - lives in buffers of its own, sized by the
 *                                 geometry.  n + the kept context may not exceed the frames max_samples allows per call.
 *   Errors: bad pointers / n < 0 / stride < n / wav_cap < 0: VC_EINVAL (checked first, NULL handle included); no open
 *   stream: VC_ESTATE; a failed call closes the stream. */
int vc_codec_stream_geometry(const vc_codec_cfg* cfg, int* lookahead_frames, int* left_context_frames, int* start_frames);
int vc_codec_decode_stream_begin(vc_codec* c);
int vc_codec_decode_stream(vc_codec* c, const int64_t* codes_dev, int stride, int n, int last, float* wav_dev,
                           int wav_cap, int* n_samples_out, void* stream);
/* ---- many decode streams on one handle, advanced together.  Up to max_batch independent streams, each holding what the single
 * stream above holds ((h, c) of both LSTM layers, kept latents, kept LSTM outputs, counters) in buffers of its own.  The single
 * stream keeps its own state: it, the streams here and the blocking calls may be interleaved on one handle.
 *   vc_codec_decode_streams_open   n in [1, max_batch] streams, ids 0 .. n - 1, all at their start (zero LSTM state); a second open
 *                                  restarts all.  More than 2 LSTM layers: VC_EINVAL, as vc_codec_decode_stream_begin.
 *   vc_codec_decode_streams_reset  puts stream `id` back at its start (and re-opens it after `last` or a failed call).  Host only,
 *                                  like open once the buffers exist: no device work, no synchronisation (the stream's first pass
 *                                  through the LSTM takes zeros for (h, c)), so it may be called while other work is queued.
 *   vc_codec_decode_streams        host arrays of n entries, no stream twice: entry i feeds stream ids[i] its next n_frames[i] frames
 *                                  (0 is legal) from codes_dev[i] (device, int64 [K][n_frames[i]], row stride stride[i]); last[i]
 *                                  flushes and closes that stream; wav_dev[i] (device, wav_cap[i] samples) receives
 *                                  n_samples_out[i] samples.  Every stream emits, bit for bit and with exactly the per-call sample
 *                                  counts, what vc_codec_decode_stream emits for the same sequence of feeds, whatever the other
 *                                  streams of the call do.  The call returns with the samples written.
 *     Every entry is planned and checked before anything is queued: on a stream id out of range or given twice, a closed stream
 *     (VC_ESTATE), a chunk over the capacity or a wav_cap too small (VC_ECAP), n_frames < 0, stride < n_frames or a null pointer
 *     (VC_EINVAL) no stream consumes anything, and the corrected call gives the right result.  A call that fails later (a code
 *     index out of range, a HIP error) closes the streams it fed.
 *     Entries whose plans coincide (frames fed and kept, frames through the LSTM, frames handed out, `last`) form a GROUP and run
 *     as ONE batched launch sequence - window assembly, first conv, LSTM with B carried states, the stack behind it, hand-out - whose
 *     launch count does not depend on the group's size, where the batched LSTM exists (2 layers, width a multiple of 256 up to
 *     1024: vc_codec_decode_batch's condition); every other entry is a group of one.  Streams fed in lock-step are one group.
 *   vc_codec_last_streams_census   of the last vc_codec_decode_streams call: out[0] groups run, out[1] size of the largest,
 *                                  out[2] kernel launches plus asynchronous copies the call queued, out[3] LSTM form of the largest
 *                                  group (vc_codec_last_forms' values; -1: nothing went through the LSTM).  out[2] is the host's
 *                                  own bookkeeping - a tally kept next to each launch site of the decode path - not an observation
 *                                  of the queue: it shows how the call was grouped and planned, it cannot prove what ran. */
int vc_codec_decode_streams_open(vc_codec* c, int n);
int vc_codec_decode_streams_reset(vc_codec* c, int id);
int vc_codec_decode_streams(vc_codec* c, int n, const int* ids, const int64_t* const* codes_dev, const int* stride,
                            const int* n_frames, const int* last, float* const* wav_dev, const int* wav_cap,
                            int* n_samples_out, void* stream);
int vc_codec_last_streams_census(const vc_codec* c, int out[4]);

/* Test hooks: the latent before quantisation ([T][hidden], channels-last) of the last encode,
 * and its timing (HIP events on the stream). */
int vc_codec_debug_latent(vc_codec* c, float* host_dst, int64_t n_floats);
int vc_codec_last_ms(const vc_codec* c, float* ms);
/* Duration of the LSTM recurrence (T+1 wavefront launches) of the last call and the weight bytes one launch reads. */
int vc_codec_last_lstm_ms(vc_codec* c, float* ms, double* bytes_per_step);
/* Which kernel forms the last calls took (-1: none yet).  lstm_form: 0 = lstm_step_k layer by layer, 1 = the two-layer
 * wavefront lstm_wave_k, 2 = the persistent lstm_persist_k (of the last encode, decode or stream chunk);
 * rvq_form: 0 = rvq_encode_k (scalar), 1 = rvq_encode_mfma_k (of the last encode). */
int vc_codec_last_forms(const vc_codec* c, int* lstm_form, int* rvq_form);

#ifdef __cplusplus
}
#endif
#endif /* VC_CODEC_H */
