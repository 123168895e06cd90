"""-m gpu: audio of a decode session's streaming requests while it decodes (voicecraft_amd.stream.SessionStreamer):
DecodeSession.poll_frames into ONE AudioTokenizer.decode_streams feed per pump.  Per ticket the concatenated audio is bit for bit
`tokenizer.decode` of the request's gen."""
import pytest
import torch

from _util import build_case
from voicecraft_amd import synth

pytestmark = pytest.mark.gpu


def test_session_streamer_audio_is_decode_of_gen():
    from voicecraft_amd import SessionStreamer
    from voicecraft_amd.codec import AudioTokenizer
    from voicecraft_amd.engine import VoiceCraftEngine
    _, args, sd, _, _, _ = build_case("tts_greedy")                         # the `tiny` model of tests/test_gpu_stream_tts.py
    eng = VoiceCraftEngine(args, sd, device="cuda:0", dtype="fp32", max_seqs=4, max_positions=512)
    eng.set_option("graph_steps", 4)
    tok = AudioTokenizer(synth.make_codec_state_dict(0), device="cuda:0", max_seconds=8.0, max_batch=4)
    prompts = [synth.random_prompt(args, 4 + u, 12 + 5 * u, seed=1300 + u) for u in range(6)]
    audio, first_audio_while_busy, done_seen = {}, [], set()
    with eng.open_session(3, top_k=1, stop_repetition=3) as sess:
        pump = SessionStreamer(sess, tok, chunk_frames=8)
        tickets = [sess.submit(*p, stream=True) for p in prompts]
        for _ in range(2000):
            for t, wav, done in pump.pump():
                assert t not in done_seen
                assert wav.ndim == 3 and wav.shape[:2] == (1, 1)
                if t not in audio and wav.shape[2]:
                    first_audio_while_busy.append(not sess.idle)
                audio.setdefault(t, []).append(wav)
                if done:
                    done_seen.add(t)
                assert len(pump.ids) <= sess.max_live
            if sess.idle and len(done_seen) == len(tickets):
                break
        results = {t: (res, gen) for t, res, gen in pump.take_results()}
        assert sess.idle and sorted(results) == sorted(tickets) == sorted(done_seen)
        assert pump.ids == {} and sorted(pump.free) == [0, 1, 2]
    assert any(first_audio_while_busy), "no audio left the session before it went idle"
    lens = set()
    for t in tickets:
        gen = results[t][1]
        assert int(gen.min()) >= 0 and int(gen.max()) < 2048, "precondition: the requests generate codec ids only"
        want = tok.decode([(gen, None)])
        got = torch.cat(audio[t], dim=2)
        assert got.shape == want.shape and torch.equal(got, want), (t, got.shape, want.shape)
        lens.add(gen.shape[2])
    assert len(lens) > 1
