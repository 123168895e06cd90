"""Streaming TTS glue: tokens from the engine's resumable decode loop into the codec's chunked decode.

`stream_tts` is what a front-end would write: it yields waveform chunks (the GENERATED part only) while the decode loop is
still running.  Concatenated, they are bit for bit `tokenizer.decode` of the `gen` a blocking `inference_tts` call with the
same arguments returns.

`SessionStreamer` does the same for every streaming request of a decode session at once: the frames `DecodeSession.poll_frames`
hands out go through ONE `CodecDecodeStreams.feed` per pump, so requests that advance in lock-step share one batched launch
sequence of the codec."""
from __future__ import annotations

import contextlib

import torch


def stream_tts(model, tokenizer, x, x_lens, y, **decode_kwargs):
    """Generator of wav fp32 [1, 1, m] chunks.  `decode_kwargs` go to `VoiceCraftEngine.inference_tts_stream` (top_k, ...,
    chunk_frames).  The codec chunks run on a stream of their own, so they overlap the decode batches the engine keeps queued.
    After exhaustion `model.last_stream_result` holds the blocking call's (res, gen)."""
    dec = tokenizer.decode_stream()
    side = torch.cuda.Stream(device=tokenizer.device)
    K = tokenizer.n_q
    tokens = model.inference_tts_stream(x, x_lens, y, **decode_kwargs)
    try:
        for _first, codes in tokens:
            if codes.shape[2] == 0:
                continue
            with torch.cuda.stream(side):
                wav = dec.feed(codes)
            if wav.shape[2]:
                yield wav
        with torch.cuda.stream(side):
            wav = dec.feed(torch.empty((1, K, 0), dtype=torch.int64, device=tokenizer.device), last=True)
        if wav.shape[2]:
            yield wav
    finally:
        tokens.close()


class SessionStreamer:
    """Audio of the streaming requests (DecodeSession.submit(..., stream=True)) of a decode session while it decodes.

    pump() runs one poll() and one poll_frames(chunk_frames) of the session, feeds everything pulled to the tokenizer's decode
    streams in ONE call and returns [(ticket, wav fp32 [1, 1, m], done)]; per ticket the concatenated audio is bit for bit
    `tokenizer.decode` of the request's `gen`.  The finished (ticket, res, gen) of every request, streaming or not, collect in
    `.results` (take them with take_results()).  A ticket holds one of `max_live` codec stream ids from its first chunk until its
    chunk with done = True; ids are reused from a free list and reset on reuse.  poll()'s SessionRequestError passes through pump();
    the failed tickets' streams are closed by the next pump.  cancel(ticket) cancels the request in the session, returns its codec
    stream id to the free list and drops a result of it waiting in `.results`.  Editing and best-of-N requests do not stream (their
    results still collect in `.results`); shared prefixes remain outside sessions."""

    def __init__(self, sess, tokenizer, chunk_frames: int = 8):
        self.sess, self.tok, self.chunk_frames = sess, tokenizer, int(chunk_frames)
        assert self.chunk_frames >= 1, chunk_frames
        self.dec = tokenizer.decode_streams(int(sess.max_live))
        self.free = list(range(int(sess.max_live)))
        self.used: set[int] = set()        # ids that have carried a clip: reset before the next one
        self.ids: dict[int, int] = {}      # ticket -> codec stream id, from its first chunk to its last
        self.results: list = []
        dev = getattr(tokenizer, "device", None)
        self._side = torch.cuda.Stream(device=dev) if getattr(dev, "type", None) == "cuda" else None

    def take_results(self):
        out, self.results = self.results, []
        return out

    def cancel(self, ticket: int) -> str:
        """DecodeSession.cancel(ticket) for a request of this streamer: the ticket gets no further audio, its codec stream id is free
        for the next ticket (reset on reuse) and a result of it waiting in `.results` is dropped ("finished")."""
        ticket = int(ticket)
        if any(r[0] == ticket for r in self.results):
            self.results = [r for r in self.results if r[0] != ticket]
            was = "finished"
        else:
            was = self.sess.cancel(ticket)
        sid = self.ids.pop(ticket, None)
        if sid is not None:
            self.free.append(sid)
        return was

    def pump(self):
        self.results += self.sess.poll()
        pulled = self.sess.poll_frames(self.chunk_frames)
        if not pulled:
            return []
        chunks, last = {}, []
        for ticket, _first, codes, done in pulled:
            sid = self.ids.get(ticket)
            if sid is None:
                sid = self.ids[ticket] = self.free.pop(0)
                if sid in self.used:
                    self.dec.reset(sid)
                self.used.add(sid)
            if codes.shape[2]:
                chunks[sid] = codes
            if done:
                last.append(sid)
        # on a stream of its own: the codec chunks overlap the decode batches the engine keeps queued (as in stream_tts)
        with (torch.cuda.stream(self._side) if self._side is not None else contextlib.nullcontext()):
            wavs = self.dec.feed(chunks, last=last)
        out = []
        for ticket, _first, _codes, done in pulled:
            sid = self.ids[ticket]
            out.append((ticket, wavs[sid], done))
            if done:
                del self.ids[ticket]
                self.free.append(sid)
        return out
