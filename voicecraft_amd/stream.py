"""Streaming TTS glue: tokens from the engine's resumable decode loop into the codec's chunked decode.

`stream_tts` is what a front-end would write: it yields waveform chunks (the GENERATED part only) while the decode loop is
still running.  Concatenated, they are bit for bit `tokenizer.decode` of the `gen` a blocking `inference_tts` call with the
same arguments returns."""
from __future__ import annotations

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
