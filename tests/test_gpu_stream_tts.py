"""-m gpu: the streaming TTS call (vc_tts_stream_begin / next / end, VoiceCraftEngine.inference_tts_stream, stream_tts)
against the blocking call.

The streamed chunks are contiguous from frame 0, every `next` delivers at least `chunk_frames` frames unless it is the last,
their concatenation is `gen` of inference_tts with the same seed and options token for token, and
`last_stream_result` is that call's (res, gen): same kernels, same captured graphs, same Philox stream.  Through the
new path the reference's golden results are reproduced as through the blocking one."""
import ctypes as C

import numpy as np
import pytest
import torch

from _util import MODEL_CASES, build_case, load_golden
from voicecraft_amd import synth
from voicecraft_amd._lib import EngineError

pytestmark = pytest.mark.gpu


def make_engine(name, dtype, **kw):
    from voicecraft_amd.engine import VoiceCraftEngine
    spec, args, sd, x, x_lens, y = build_case(name)
    eng = VoiceCraftEngine(args, sd, device="cuda:0", dtype=dtype, max_seqs=4, max_positions=512, **kw)
    return eng, spec, x.cuda(), x_lens.cuda(), y.cuda()


def consume(eng, x, x_lens, y, chunk, **kw):
    """-> (concatenated gen [1,K,Tg], list of (first, n)); asserts contiguity and the minimum chunk size"""
    chunks, at = [], 0
    for first, codes in eng.inference_tts_stream(x, x_lens, y, chunk_frames=chunk, **kw):
        assert first == at, (first, at)
        assert codes.ndim == 3 and codes.shape[0] == 1 and codes.shape[1] == eng.args.n_codebooks
        chunks.append(codes)
        at += codes.shape[2]
    sizes = [int(c.shape[2]) for c in chunks]
    assert all(n >= chunk for n in sizes[:-1]), (chunk, sizes)          # only the last chunk may be short
    K = eng.args.n_codebooks
    cat = torch.cat(chunks, dim=2) if chunks else torch.empty((1, K, 0), dtype=torch.int64, device=x.device)
    return cat, sizes


@pytest.fixture(scope="module", params=["fp32", "bf16"])
def eng_case(request):
    return make_engine("tts_greedy", request.param)


@pytest.mark.parametrize("graph_steps", [1, 8])
@pytest.mark.parametrize("knobs", [dict(top_k=1), dict(top_k=40, top_p=1.0, temperature=1.0)], ids=["greedy", "topk40"])
def test_streamed_tokens_equal_the_blocking_call(eng_case, knobs, graph_steps):
    eng, spec, x, x_lens, y = eng_case
    eng.set_option("graph_steps", graph_steps)
    kw = dict(knobs, stop_repetition=3, _seed=1234)
    res, gen = eng.inference_tts(x, x_lens, y, **kw)
    steps = eng.last_steps
    assert gen.shape[2] > 30
    for chunk in (1, 8, 50):
        cat, sizes = consume(eng, x, x_lens, y, chunk, **kw)
        assert torch.equal(cat, gen), (chunk, sizes)
        r2, g2 = eng.last_stream_result
        assert torch.equal(r2, res) and torch.equal(g2, gen)
        assert eng.last_steps == steps
        if chunk == 1:
            assert len(sizes) > 3          # frames really arrive in several pieces (one per graph batch), not at the end
    res_b, gen_b = eng.inference_tts(x, x_lens, y, **kw)      # and the blocking call is what it was
    assert torch.equal(res_b, res)


GREEDY_CASES = ["tts_greedy", "tts_oldscheme", "tts_eos_greedy", "tts_eos_guard", "tts_early_stop"]
DRAW_CASES = ["tts_sampled", "tts_sampled_eos"]


@pytest.mark.parametrize("graph_steps", [1, 8])
@pytest.mark.parametrize("name", GREEDY_CASES + DRAW_CASES)
def test_reference_parity_through_the_stream(name, graph_steps):
    """fp32: the reference's `res` - both special-token schemes, an arg-max terminator in the middle, the min-length guard
    releasing after about one graph batch, a prompt already past the length cap (done at the first `next`), and the
    reference's own draws replayed through the state machine."""
    g = load_golden(name)
    eng, spec, x, x_lens, y = make_engine(name, "fp32")
    eng.set_option("graph_steps", graph_steps)
    kn = dict(spec["knobs"])
    extra = dict(_forced=g["draws"], _forced_mode="draws", _seed=99) if name in DRAW_CASES else dict(_seed=1)
    cat, sizes = consume(eng, x, x_lens, y, 4, **kn, **extra)
    res, gen = eng.last_stream_result
    assert list(res.shape) == list(g["res"].shape), (res.shape, g["res"].shape)
    assert np.array_equal(res.cpu().numpy(), g["res"])
    assert torch.equal(cat, gen) and gen.shape[2] == res.shape[2] - y.shape[1]
    if name == "tts_early_stop":
        assert len(sizes) <= 1, sizes


def _launched(eng):
    return int(eng.debug_read("host_ms", (8,), torch.float64)[5])


@pytest.mark.parametrize("use_graph", [True, False])
def test_the_stream_does_the_blocking_calls_work(use_graph):
    """Same steps taken and same steps LAUNCHED (a multiple of graph_steps) as the blocking call.  The census of kernel forms
    counts what is launched outside a graph replay: with the graph on that is the prefill plus any CAPTURE of decode steps, so
    a streamed call behind a blocking one of the same shape must add exactly what a repeated blocking call adds (the prefill;
    no capture of its own); with the graph off it counts every decode launch, and the two calls must agree form by form."""
    eng, spec, x, x_lens, y = make_engine("tts_greedy", "bf16", use_graph=use_graph)
    kw = dict(top_k=40, stop_repetition=3, _seed=7)
    eng.inference_tts(x, x_lens, y, **kw)                    # the first call of the shape captures
    c0 = eng.launch_counts()
    eng.inference_tts(x, x_lens, y, **kw)
    c1 = eng.launch_counts()
    steps, launched = eng.last_steps, _launched(eng)
    assert launched % 8 == 0 and launched >= steps - 1
    consume(eng, x, x_lens, y, 8, **kw)
    c2 = eng.launch_counts()
    assert eng.last_steps == steps and _launched(eng) == launched
    blocking, streamed = {k: c1[k] - c0[k] for k in c1}, {k: c2[k] - c1[k] for k in c2}
    assert streamed == blocking, (streamed, blocking)
    assert sum(blocking.values()) > 0
    if not use_graph:
        assert sum(blocking.values()) > launched             # every decode step's launches are in the census


def test_stream_state_machine():
    eng, spec, x, x_lens, y = make_engine("tts_greedy", "fp32")
    kw = dict(top_k=1, stop_repetition=3, _seed=1)
    res, gen = eng.inference_tts(x, x_lens, y, **kw)
    it = eng.inference_tts_stream(x, x_lens, y, chunk_frames=8, **kw)
    first, codes = next(it)
    assert first == 0 and torch.equal(codes, gen[:, :, : codes.shape[2]]) and codes.shape[2] >= 8
    with pytest.raises(EngineError, match="streaming TTS call is open"):          # VC_ESTATE
        eng.inference_tts(x, x_lens, y, **kw)
    with pytest.raises(EngineError, match="streaming TTS call is open"):
        next(eng.inference_tts_stream(x, x_lens, y, **kw))
    with pytest.raises(EngineError, match="streaming TTS call is open"):
        eng.set_option("graph_steps", 4)
    it.close()                                                                    # abort after the first chunk
    assert eng.last_stream_result is None
    res2, gen2 = eng.inference_tts(x, x_lens, y, **kw)                            # the engine is usable and gives its usual tokens
    assert torch.equal(res2, res)
    cat, _ = consume(eng, x, x_lens, y, 8, **kw)                                  # ... and so does a new stream
    assert torch.equal(cat, gen)
    with pytest.raises(AssertionError, match="best-of-N"):
        eng.inference_tts_stream(x, x_lens, y, _n_samples=3, **kw)
    # next / end without an open stream
    n = C.c_int(0)
    buf = torch.empty((4, 16), dtype=torch.int64, device="cuda")
    rc = eng.lib.vc_tts_stream_next(eng._h, 1, C.c_void_p(buf.data_ptr()), 16, C.byref(n), C.byref(n), C.byref(n))
    assert rc == -2
    assert eng.lib.vc_tts_stream_end(eng._h, None, 0, None, None) == -2


def test_stream_tts_audio_equals_decode_of_the_blocking_tokens():
    from voicecraft_amd import stream_tts
    from voicecraft_amd.codec import AudioTokenizer
    tok = AudioTokenizer(synth.make_codec_state_dict(0), device="cuda:0", max_seconds=8.0)
    for dtype in ("fp32", "bf16"):
        eng, spec, x, x_lens, y = make_engine("tts_greedy", dtype)
        kw = dict(top_k=40, stop_repetition=3, _seed=5)
        res, gen = eng.inference_tts(x, x_lens, y, **kw)
        assert int(gen.min()) >= 0 and int(gen.max()) < 2048, "precondition: the case generates codec ids only"
        want = tok.decode([(gen, None)])
        chunks = list(stream_tts(eng, tok, x, x_lens, y, chunk_frames=8, **kw))
        assert len(chunks) > 2
        assert torch.equal(torch.cat(chunks, dim=2), want)
        assert torch.equal(eng.last_stream_result[1], gen)
