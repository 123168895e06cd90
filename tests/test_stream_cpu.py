"""Streaming, the part that needs no GPU: argument validation of the six new entry points (chunked codec decode,
resumable TTS call) and the stream geometry (vc_codec_stream_geometry) against the transformers.EncodecModel restatement.

The geometry is checked the way a stream relies on it.  Perturbing the CODES of one interior frame p must change no
sample of frames < p - lookahead (the look-ahead is sufficient: those samples were final when they were emitted) and
must change a sample of frame p - lookahead (it is tight to the frame).  Behind the LSTM, perturbing the LSTM output
of frame p must change no sample of frames >= p + left_context and none of frames < p - right (right = lookahead minus
the first conv's right taps), and must reach frames p + left_context - 1 and p - right."""
import ctypes as C

import pytest
import torch

from oracle import encodec_oracle as eo
from voicecraft_amd import synth
from voicecraft_amd import codec as vcodec

HOP = 320
CONFIGS = [dict(), dict(use_causal_conv=True), dict(pad_mode="constant"), dict(use_conv_shortcut=True),
           dict(num_residual_layers=2, dilation_growth_rate=2),
           dict(use_causal_conv=True, pad_mode="constant", use_conv_shortcut=True)]
IDS = lambda k: "+".join(f"{a}={b}" for a, b in k.items()) or "default"      # noqa: E731


@pytest.fixture(scope="module")
def lib():
    return vcodec._bind(vcodec._lib.load())


def test_argument_validation_without_a_device(lib):
    cfg = vcodec.make_cfg()
    la, lc, st = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert lib.vc_codec_stream_geometry(None, C.byref(la), C.byref(lc), C.byref(st)) == -1
    assert lib.vc_codec_stream_geometry(C.byref(cfg), None, C.byref(lc), C.byref(st)) == -1
    assert lib.vc_codec_stream_geometry(C.byref(cfg), C.byref(la), None, C.byref(st)) == -1
    assert lib.vc_codec_stream_geometry(C.byref(cfg), C.byref(la), C.byref(lc), None) == 0        # start_frames is optional
    bad = vcodec.make_cfg()
    bad.n_ratios = 0
    assert lib.vc_codec_stream_geometry(C.byref(bad), C.byref(la), C.byref(lc), C.byref(st)) == -1
    bad = vcodec.make_cfg(dict(num_residual_layers=9))
    assert lib.vc_codec_stream_geometry(C.byref(bad), C.byref(la), C.byref(lc), C.byref(st)) == -1
    assert lib.vc_codec_decode_stream_begin(None) == -1
    buf = (C.c_int64 * 16)()
    wav = (C.c_float * 16)()
    n = C.c_int(0)
    p, w = C.cast(buf, C.c_void_p), C.cast(wav, C.c_void_p)
    call = lib.vc_codec_decode_stream
    assert call(None, p, 4, -1, 0, w, 16, C.byref(n), None) == -1          # n < 0
    assert call(None, None, 4, 4, 0, w, 16, C.byref(n), None) == -1        # frames without codes
    assert call(None, p, 3, 4, 0, w, 16, C.byref(n), None) == -1           # stride < n
    assert call(None, p, 4, 4, 0, None, 16, C.byref(n), None) == -1        # no output buffer
    assert call(None, p, 4, 4, 0, w, -1, C.byref(n), None) == -1           # negative capacity
    assert call(None, p, 4, 4, 0, w, 16, None, None) == -1                 # nowhere to report the count
    assert call(None, p, 4, 4, 0, w, 16, C.byref(n), None) == -2           # valid arguments, but no codec: VC_ESTATE
    assert call(None, None, 0, 0, 1, w, 16, C.byref(n), None) == -2        # an empty final call is a valid call


def test_tts_stream_argument_validation_without_a_device():
    """vc_tts_stream_begin / next / end: bad pointers, cap < 1, min_frames < 1 (or > cap) are VC_EINVAL before anything
    touches a device - exercised with a NULL engine, as the pattern calls are."""
    from voicecraft_amd import _lib
    lib = _lib.load()
    sc = _lib.SampleCfg(top_k=1, top_p=1.0, temperature=1.0)
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    begin, nxt, end = lib.vc_tts_stream_begin, lib.vc_tts_stream_next, lib.vc_tts_stream_end
    assert begin(None, None, 4, p, 2, C.byref(sc), None, 0, None) == -1          # no text
    assert begin(None, p, 4, None, 2, C.byref(sc), None, 0, None) == -1          # prompt frames without a prompt
    assert begin(None, p, 4, p, 2, None, None, 0, None) == -1                    # no sampling config
    assert begin(None, p, 0, p, 2, C.byref(sc), None, 0, None) == -1             # empty text
    assert begin(None, p, 4, p, 2, C.byref(sc), None, 0, None) == -1             # valid arguments, NULL engine
    assert nxt(None, 1, None, 16, C.byref(a), C.byref(b), C.byref(c)) == -1
    assert nxt(None, 1, p, 0, C.byref(a), C.byref(b), C.byref(c)) == -1          # cap < 1
    assert nxt(None, 0, p, 16, C.byref(a), C.byref(b), C.byref(c)) == -1         # min_frames < 1
    assert nxt(None, 17, p, 16, C.byref(a), C.byref(b), C.byref(c)) == -1        # min_frames > cap could never be met
    assert nxt(None, 1, p, 16, None, C.byref(b), C.byref(c)) == -1
    assert nxt(None, 1, p, 16, C.byref(a), None, C.byref(c)) == -1
    assert nxt(None, 1, p, 16, C.byref(a), C.byref(b), None) == -1
    assert b"vc_tts_stream_next" in lib.vc_last_error(None)
    assert end(None, p, 16, None, None) == -1                                    # a result buffer without gen_len
    assert end(None, None, 0, None, None) == -1                                  # NULL engine


def test_geometry_of_the_voicecraft_codec_shape():
    # derived by the oracle test below; pinned here so a change of the derivation is seen at a glance
    assert vcodec.stream_geometry() == (4, 2, 4)
    assert vcodec.stream_geometry(dict(use_causal_conv=True)) == (0, 3, 7)
    assert vcodec.stream_geometry(dict(use_causal_conv=True, pad_mode="constant")) == (0, 3, 1)
    assert vcodec.stream_geometry(dict(num_residual_layers=2, dilation_growth_rate=2)) == (5, 3, 4)
    assert vcodec.stream_geometry(dict(pad_mode="constant"))[2] == 1


def _changed_frames(a, b):
    d = (a != b).reshape(-1, HOP).any(dim=1)
    return [int(i) for i in d.nonzero().flatten()]


@torch.no_grad()
def _decode_with_lstm_bump(m, codes, p):
    """decoder output with the LSTM block's output of frame p perturbed (p < 0: untouched)"""
    x = m.quantizer.decode(codes.unsqueeze(1))
    for i, layer in enumerate(m.decoder.layers):
        x = layer(x)
        if i == 1 and p >= 0:
            x = x.clone()
            x[:, :, p] += 0.5
    return x[0, 0]


@pytest.mark.parametrize("kw", CONFIGS, ids=IDS)
def test_geometry_is_sufficient_and_tight_against_the_oracle(kw):
    sd = synth.make_codec_state_dict(2, use_conv_shortcut=kw.get("use_conv_shortcut", False),
                                     num_residual_layers=kw.get("num_residual_layers", 1))
    m = eo.build(sd, **kw)
    lookahead, left, start = vcodec.stream_geometry(kw)
    k = vcodec.DEFAULT_CFG["kernel_size"]
    right = lookahead - (0 if kw.get("use_causal_conv") else (k - 1) // 2)     # what is left of it behind the LSTM
    assert lookahead >= 0 and left >= 1 and right >= 0 and start >= 1
    T, p = 80, 40
    g = torch.Generator().manual_seed(11)
    codes = torch.randint(0, 2048, (4, T), generator=g)
    base = eo.decode(m, codes)
    # ---- look-ahead: the codes of frame p
    other = codes.clone()
    other[:, p] = (other[:, p] + 977) % 2048
    ch = _changed_frames(base, eo.decode(m, other))
    print(kw, "codes of frame", p, "changed frames", ch[0], "..", ch[-1], "lookahead", lookahead)
    assert ch[0] >= p - lookahead, (ch[0], lookahead)                  # sufficient
    assert ch[0] == p - lookahead, (ch[0], lookahead)                  # tight to the frame (lookahead 0: frame p itself)
    # ---- behind the LSTM: the LSTM output of frame p
    ref = _decode_with_lstm_bump(m, codes, -1)
    assert torch.equal(ref, base)
    ch = _changed_frames(ref, _decode_with_lstm_bump(m, codes, p))
    print(kw, "LSTM output of frame", p, "reaches frames", ch[0], "..", ch[-1], "left", left, "right", right)
    assert ch[-1] <= p + left - 1 and ch[0] >= p - right, (ch, left, right)      # sufficient
    assert ch[-1] == p + left - 1 and ch[0] == p - right, (ch, left, right)      # tight


def test_start_frames_cover_the_reflect_padding_at_the_true_start():
    """With reflect padding the first frames mirror the ones behind them (frame 0 of a causal codec reads frame 6), and
    a clip no longer than the padding is zero-extended first: until start_frames frames are known nothing may leave.
    Oracle: changing frame start_frames - 1 changes frame 0's samples, so a stream that emitted frame 0 earlier would
    have been wrong."""
    kw = dict(use_causal_conv=True)
    m = eo.build(synth.make_codec_state_dict(2), **kw)
    lookahead, _, start = vcodec.stream_geometry(kw)
    assert lookahead == 0 and start == 7
    g = torch.Generator().manual_seed(5)
    codes = torch.randint(0, 2048, (4, 30), generator=g)
    other = codes.clone()
    other[:, start - 1] = (other[:, start - 1] + 5) % 2048
    assert 0 in _changed_frames(eo.decode(m, codes), eo.decode(m, other))
