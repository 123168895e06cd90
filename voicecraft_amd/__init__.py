"""voicecraft_amd — MI355X-native engine for VoiceCraft's token-infilling decode path.

Public surface (mirrors the reference's model interface):
    VoiceCraftEngine.inference_tts / inference_tts_batch / inference
    pattern_shift / pattern_revert / pattern_unshift   (delayed-codebook pattern, bit-exact)
    AudioTokenizer                                     (EnCodec encode/decode, .decode_stream())
    VoiceCraftEngine.inference_tts_stream, stream_tts  (tokens / audio while the decode loop runs)
    VoiceCraftEngine.open_session -> DecodeSession, inference_tts_queue, inference_queue
                                                       (continuous batching: TTS and editing requests join a running batch)
    DecodeSession.submit(stream=True) / poll_frames, AudioTokenizer.decode_streams, SessionStreamer
                                                       (frames and audio of every streaming request while the session decodes)
    DecodeSession.cancel / SessionStreamer.cancel      (a pending, live or finished request leaves the session)
Everything computes in libvcengine.so (HIP, gfx950); importing this package does not need a GPU,
constructing an engine does.
"""
from .synth import PRESETS, make_args, make_state_dict, random_prompt  # noqa: F401


def __getattr__(name):
    if name in ("VoiceCraftEngine", "DecodeSession", "SessionRequestError", "inference_tts_queue", "inference_queue", "pattern_shift", "pattern_revert", "pattern_unshift"):
        from . import engine
        return getattr(engine, name)
    if name in ("stream_tts", "SessionStreamer"):
        from . import stream
        return getattr(stream, name)
    if name == "AudioTokenizer":
        from . import codec
        return codec.AudioTokenizer
    raise AttributeError(name)
