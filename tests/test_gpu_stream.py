"""-m gpu: the chunked codec decode (vc_codec_decode_stream) against the one-shot call.

Contract: whatever way a code sequence is split into chunks, the concatenation of what the stream emits is BIT FOR BIT
`tokenizer.decode` of the whole sequence, and every chunk has exactly the length the geometry promises (nothing
emitted early, nothing withheld past the look-ahead).  A persistent-LSTM hand-off wait that gave up would fail the
call (check_lstm_flag -> VC_EHIP), so every passing feed also asserts that the error path did not fire."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import encodec_oracle as eo
from voicecraft_amd import synth
from voicecraft_amd._lib import EngineError

pytestmark = pytest.mark.gpu

HOP = 320
LENGTHS = [1, 3, 4, 5, 9, 50, 173]
SPLITS = ["ones", "eights", "whole", "random", "empty_last"]


def _split(kind, T, seed=0):
    """-> list of chunk sizes; the final entry is the call with last=True"""
    if kind == "ones":
        return [1] * T
    if kind == "eights":
        return [8] * (T // 8) + ([T % 8] if T % 8 else [])
    if kind == "whole":
        return [T]
    if kind == "empty_last":
        return [8] * (T // 8) + ([T % 8] if T % 8 else []) + [0]
    rs, out, left = np.random.RandomState(seed), [], T
    while left:
        n = int(rs.randint(1, 14))
        out.append(min(n, left))
        left -= out[-1]
    return out


def _codes(T, seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 2048, size=(1, 4, T)).astype(np.int64)).cuda()


def _stream_decode(tok, codes, sizes, between=None):
    """feeds `codes` in chunks of `sizes`; checks every chunk's length against the promise; -> the concatenation"""
    st = tok.decode_stream()
    out, fed = [], 0
    for i, n in enumerate(sizes):
        last = i == len(sizes) - 1
        before = st.emitted
        w = st.feed(codes[:, :, fed: fed + n], last=last)
        fed += n
        want = fed * HOP if last else st.ready_frames(fed) * HOP
        assert w.shape == (1, 1, want - before), (i, n, w.shape, want, before)
        out.append(w)
        if between is not None:
            between(i)
    assert st.closed and st.emitted == fed * HOP
    return torch.cat(out, dim=2)


@pytest.fixture(scope="module")
def tok():
    from voicecraft_amd.codec import AudioTokenizer
    return AudioTokenizer(synth.make_codec_state_dict(0), device="cuda:0", max_seconds=8.0)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("T", LENGTHS)
def test_stream_equals_the_one_shot_decode_bit_for_bit(tok, T, split):
    codes = _codes(T, T)
    want = tok.decode([(codes, None)])
    got = _stream_decode(tok, codes, _split(split, T, seed=T))
    assert got.shape == want.shape
    assert torch.equal(got, want), float((got - want).abs().max())


@pytest.mark.parametrize("env", ["VC_LSTM_WAVE", "VC_LSTM_SEQUENTIAL"])
@pytest.mark.parametrize("T", [3, 9, 50])
def test_stream_on_the_launch_per_step_lstm_forms(tok, T, env, monkeypatch):
    """The carried state goes through all three forms of the recurrence: the persistent launch (default, above), the
    two-layer wavefront (VC_LSTM_WAVE=1) and the sequential per-layer steps (VC_LSTM_SEQUENTIAL=1)."""
    codes = _codes(T, 100 + T)
    monkeypatch.setenv(env, "1")
    want = tok.decode([(codes, None)])
    for split in ("ones", "random", "empty_last"):
        assert torch.equal(_stream_decode(tok, codes, _split(split, T, seed=T)), want), split
    monkeypatch.delenv(env)
    if env == "VC_LSTM_WAVE":       # and the persistent stream equals the wavefront one-shot (same order of every sum)
        assert torch.equal(_stream_decode(tok, codes, _split("eights", T)), want)


VARIANTS = [dict(use_causal_conv=True), dict(pad_mode="constant"), dict(num_residual_layers=2, dilation_growth_rate=2),
            dict(use_causal_conv=True, pad_mode="constant", use_conv_shortcut=True)]


@pytest.mark.parametrize("kw", VARIANTS, ids=lambda k: "+".join(f"{a}={b}" for a, b in k.items()))
def test_stream_with_architecture_switches(kw):
    """The geometry follows the config: causal has no look-ahead (but, with reflect padding, a start of 7 frames), two
    residual units reach further.  Same contract, and the stream stays inside the codec's bar against the oracle."""
    from voicecraft_amd.codec import AudioTokenizer, stream_geometry
    sd = synth.make_codec_state_dict(2, use_conv_shortcut=kw.get("use_conv_shortcut", False),
                                     num_residual_layers=kw.get("num_residual_layers", 1))
    t = AudioTokenizer(sd, device="cuda:0", max_seconds=2.0, cfg=kw, max_batch=1)
    la, _, start = stream_geometry(kw)
    assert t.decode_stream().lookahead_frames == la
    for T in (1, 5, 7, 8, 41):
        codes = _codes(T, 7 + T)
        want = t.decode([(codes, None)])
        for split in ("ones", "random", "whole", "empty_last"):
            got = _stream_decode(t, codes, _split(split, T, seed=3))
            assert torch.equal(got, want), (T, split, float((got - want).abs().max()))
    ref = eo.decode(eo.build(sd, **kw), codes[0].cpu()).numpy()
    rms = float(np.sqrt((ref ** 2).mean()))
    assert np.abs(got[0, 0].cpu().numpy() - ref).max() <= 2e-4 * rms + 1e-5


def test_stream_against_the_cpu_oracle(tok):
    T = 60
    codes = _codes(T, 9)
    got = _stream_decode(tok, codes, _split("eights", T))[0, 0].cpu().numpy()
    want = eo.decode(eo.build(synth.make_codec_state_dict(0)), codes[0].cpu()).numpy()
    rms = float(np.sqrt((want ** 2).mean()))
    assert np.abs(got - want).max() <= 2e-4 * rms + 1e-5, (np.abs(got - want).max(), rms)


def test_blocking_calls_between_two_feeds_do_not_disturb_the_stream(tok):
    T = 50
    codes = _codes(T, 21)
    want = tok.decode([(codes, None)])
    other = _codes(33, 22)
    other_wav = tok.decode([(other, None)])
    wav_in = (torch.randn(1, 1, 9000) * 0.1).cuda()
    other_codes = tok.encode(wav_in)[0][0]

    def between(i):
        if i % 2:
            assert torch.equal(tok.decode([(other, None)]), other_wav)
        else:
            assert torch.equal(tok.encode(wav_in)[0][0], other_codes)

    assert torch.equal(_stream_decode(tok, codes, _split("random", T, seed=2), between=between), want)


def test_stream_state_machine(tok):
    codes = _codes(20, 1)
    want = tok.decode([(codes, None)])
    st = tok.decode_stream()
    st.feed(codes[:, :, :10])
    st2 = tok.decode_stream()                        # a second begin restarts the handle's stream
    got = torch.cat([st2.feed(codes[:, :, :7]), st2.feed(codes[:, :, 7:], last=True)], dim=2)
    assert torch.equal(got, want)
    with pytest.raises(EngineError):                 # closed on the Python side
        st2.feed(codes[:, :, :1])
    n = C.c_int(0)
    wav = torch.empty(HOP * 20, device="cuda")
    cd = codes[0].contiguous()
    call = tok.lib.vc_codec_decode_stream
    rc = call(tok._h, C.c_void_p(cd.data_ptr()), 20, 20, 1, C.c_void_p(wav.data_ptr()), HOP * 20, C.byref(n), None)
    assert rc == -2 and b"no decode stream" in tok.lib.vc_codec_last_error(tok._h)          # VC_ESTATE: closed by `last`
    # a capacity that is too small consumes nothing: the same call with room succeeds and gives the whole clip
    tok._check(tok.lib.vc_codec_decode_stream_begin(tok._h), "begin")
    rc = call(tok._h, C.c_void_p(cd.data_ptr()), 20, 20, 1, C.c_void_p(wav.data_ptr()), HOP * 20 - 1, C.byref(n), None)
    assert rc == -4
    rc = call(tok._h, C.c_void_p(cd.data_ptr()), 20, 20, 1, C.c_void_p(wav.data_ptr()), HOP * 20, C.byref(n), None)
    assert rc == 0 and n.value == HOP * 20
    assert torch.equal(wav.reshape(1, 1, -1), want)
    # codes with a row stride: a [K][cap] block of which n columns are fed
    wide = torch.zeros((4, 64), dtype=torch.int64, device="cuda")
    wide[:, :20] = cd
    tok._check(tok.lib.vc_codec_decode_stream_begin(tok._h), "begin")
    rc = call(tok._h, C.c_void_p(wide.data_ptr()), 64, 20, 1, C.c_void_p(wav.data_ptr()), HOP * 20, C.byref(n), None)
    assert rc == 0 and torch.equal(wav.reshape(1, 1, -1), want)
    bad = codes.clone()
    bad[0, 0, 3] = 4096
    st = tok.decode_stream()
    with pytest.raises(AssertionError):
        st.feed(bad, last=True)
    assert torch.equal(tok.decode([(codes, None)]), want)          # the codec is still usable
