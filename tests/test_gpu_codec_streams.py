"""-m gpu: many decode streams on one codec handle, advanced together (include/vc_codec.h vc_codec_decode_streams*).

Contract: every stream emits, bit for bit and with exactly the per-call sample counts the geometry promises, what the single
stream emits for the same feeds - so its concatenation is `tokenizer.decode` of its codes - whatever the other streams of the call
are doing; streams whose plans coincide run as ONE batched launch sequence whose launch count does not depend on their number."""
import ctypes as C

import numpy as np
import pytest
import torch

import codec_shapes as cs
from test_gpu_stream import VARIANTS, _split
from voicecraft_amd import synth
from voicecraft_amd._lib import EngineError

pytestmark = pytest.mark.gpu

LENGTHS = [1, 4, 9, 41, 50]
SPLITS = ["ones", "eights", "random", "empty_last"]
_TOKS = {}


def _tok(name, max_batch=4):
    """name: "voicecraft", a codec_shapes row, or "variant<i>" of tests/test_gpu_stream.py's architecture switches."""
    from voicecraft_amd.codec import AudioTokenizer, DEFAULT_CFG
    key = (name, max_batch)
    if key not in _TOKS:
        if name in cs.CONFIGS:
            cfg = cs.CONFIGS[name]
            sd = synth.make_codec_state_dict(cs.SEED[name], cfg=cfg)
        elif name.startswith("variant"):
            cfg = VARIANTS[int(name[7:])]
            sd = synth.make_codec_state_dict(2, use_conv_shortcut=cfg.get("use_conv_shortcut", False),
                                             num_residual_layers=cfg.get("num_residual_layers", 1))
        else:
            cfg, sd = {}, synth.make_codec_state_dict(0)
        full = dict(DEFAULT_CFG, **cfg)
        hop = int(np.prod(full["ratios"]))
        tok = AudioTokenizer(sd, device="cuda:0", max_seconds=70 * hop / full["sample_rate"], cfg=cfg, max_batch=max_batch)
        _TOKS[key] = (tok, full)
    return _TOKS[key]


def _codes(full, T, seed):
    rs = np.random.RandomState(seed)
    return torch.from_numpy(rs.randint(0, full["codebook_size"], size=(1, full["n_q"], T)).astype(np.int64)).cuda()


def _run(tok, st, clips, sizes, starts=None, ids=None, between=None, census=None):
    """Stream k (id ids[k]) gets clips[k] in chunks of sizes[k], its first chunk in call starts[k]; every call feeds all the streams
    that have a chunk due in ONE feed.  Checks every chunk's length against the geometry; -> the concatenation per stream."""
    n = len(clips)
    starts = starts or [0] * n
    ids = ids or list(range(n))
    out, fed = [[] for _ in range(n)], [0] * n
    calls = max(s + len(z) for s, z in zip(starts, sizes))
    for j in range(calls):
        chunks, last, due = {}, [], []
        for k in range(n):
            i = j - starts[k]
            if 0 <= i < len(sizes[k]):
                chunks[ids[k]] = clips[k][:, :, fed[k]: fed[k] + sizes[k][i]]
                if i == len(sizes[k]) - 1:
                    last.append(ids[k])
                due.append((k, sizes[k][i], i == len(sizes[k]) - 1))
        before = {k: st.emitted[ids[k]] for k, _, _ in due}
        got = st.feed(chunks, last=last)
        for k, m, is_last in due:
            fed[k] += m
            want = fed[k] * tok.hop if is_last else st.ready_frames(fed[k]) * tok.hop
            w = got[ids[k]]
            assert w.shape == (1, 1, want - before[k]), (j, k, m, w.shape, want, before[k])
            out[k].append(w)
        if census is not None:
            census.append(st.census())
        if between is not None:
            between(j)
    for k in range(n):
        assert st.closed[ids[k]] and st.emitted[ids[k]] == fed[k] * tok.hop
    return [torch.cat(o, dim=2) for o in out]


NAMES = ["voicecraft", "half", "narrow", "w768", "seq", "variant0", "variant1", "variant2", "variant3"]


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("name", NAMES)
def test_every_stream_is_bit_equal_to_its_one_shot_decode(name, n):
    """A different length and a different split per stream, the feeds interleaved in one call sequence."""
    tok, full = _tok(name)
    clips = [_codes(full, LENGTHS[(k + n) % 5], 10 * n + k) for k in range(n)]
    want = [tok.decode([(c, None)]) for c in clips]
    sizes = [_split(SPLITS[(k + n) % 4], c.shape[2], seed=k + 1) for k, c in enumerate(clips)]
    census = []
    got = _run(tok, tok.decode_streams(n), clips, sizes, census=census)
    for k in range(n):
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), (k, clips[k].shape, float((got[k] - want[k]).abs().max()))
    if name == "seq":          # LSTM width 128, one layer: no batched form, every entry a group of one
        assert all(c[1] <= 1 for c in census) and any(c[0] > 1 for c in census), census


def test_eight_streams_on_half():
    tok, full = _tok("half", 8)
    clips = [_codes(full, LENGTHS[k % 5], 300 + k) for k in range(8)]
    want = [tok.decode([(c, None)]) for c in clips]
    sizes = [_split(SPLITS[k % 4], c.shape[2], seed=k + 1) for k, c in enumerate(clips)]
    got = _run(tok, tok.decode_streams(8), clips, sizes)
    for k in range(8):
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("wave", [False, True])
@pytest.mark.parametrize("name,batch", [("half", 16), ("voicecraft", 4)])
def test_lock_step_streams_are_one_group_whose_launch_count_does_not_depend_on_its_size(name, batch, wave, monkeypatch):
    tok, full = _tok(name, batch)
    if wave:
        monkeypatch.setenv("VC_LSTM_WAVE", "1")
    queued = {}
    # (9 streams: more than the persistent form advances per hand-off round - a second round, and a strided copy of 9 rows)
    for n in ([2, 4, 9] if batch >= 9 else [2, 4]):
        clips = [_codes(full, 48, 500 + k) for k in range(n)]
        want = [tok.decode([(c, None)]) for c in clips]
        census = []
        got = _run(tok, tok.decode_streams(n), clips, [[8] * 6] * n, census=census)
        for k in range(n):
            assert torch.equal(got[k], want[k]), (n, k)
        for c in census[2:]:
            assert c[0] == 1 and c[1] == n, (n, census)
            assert c[3] == (1 if wave else 2), (n, census)      # the wavefront when forced, else the carried persistent form
        queued[n] = [c[2] for c in census]
    assert all(q == queued[2] for q in queued.values()), queued


def test_staggered_streams():
    """Stream 1 starts when stream 0 is half way; stream 0 ends in a call in which stream 1 continues."""
    tok, full = _tok("voicecraft")
    clips = [_codes(full, 48, 600), _codes(full, 48, 601)]
    want = [tok.decode([(c, None)]) for c in clips]
    census = []
    got = _run(tok, tok.decode_streams(2), clips, [[8] * 6, [8] * 6], starts=[0, 3], census=census)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert census[5][0] == 2, census              # stream 0's last call: not the plan of stream 1, two groups


def test_reset_leaves_nothing_of_the_previous_clip():
    tok, full = _tok("voicecraft")
    st = tok.decode_streams(2)
    a, b, c2 = _codes(full, 41, 700), _codes(full, 30, 701), _codes(full, 37, 702)
    want = [tok.decode([(z, None)]) for z in (a, b, c2)]
    got = _run(tok, st, [a, b], [_split("eights", 41), _split("random", 30, seed=4)])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(EngineError, match="closed"):
        st.feed({0: c2[:, :, :8]})
    st.reset(0)
    # ... and a stream abandoned half way
    st.reset(1)
    st.feed({1: b[:, :, :17]})
    st.reset(1)
    got = _run(tok, st, [c2, b], [_split("eights", 37), _split("ones", 30)], ids=[0, 1])
    assert torch.equal(got[0], want[2]) and torch.equal(got[1], want[1])
    # a call that fails behind the validation (a code index outside the codebook) closes the streams it fed, on both sides
    st.reset(0)
    st.reset(1)
    bad = c2.clone()
    bad[0, 1, 3] = full["codebook_size"]
    with pytest.raises(AssertionError, match="code index"):
        st.feed({0: bad[:, :, :8], 1: b[:, :, :8]})
    assert st.closed == [True, True]
    with pytest.raises(EngineError, match="closed"):
        st.feed({1: b[:, :, 8:16]})
    st.reset(0)
    st.reset(1)
    got = _run(tok, st, [c2, b], [_split("random", 37, seed=5), _split("eights", 30)], ids=[0, 1])
    assert torch.equal(got[0], want[2]) and torch.equal(got[1], want[1])


def test_the_single_stream_and_blocking_calls_between_two_feeds():
    tok, full = _tok("voicecraft")
    clips = [_codes(full, 50, 800 + k) for k in range(3)]
    solo, other = _codes(full, 44, 810), _codes(full, 33, 811)
    want = [tok.decode([(c, None)]) for c in clips]
    want_solo, want_other = tok.decode([(solo, None)]), tok.decode([(other, None)])
    one = tok.decode_stream()
    solo_out = []

    def between(j):
        if j < 9:
            solo_out.append(one.feed(solo[:, :, 4 * j: 4 * j + 4]))
        if j % 3 == 0:
            assert torch.equal(tok.decode([(other, None)]), want_other)
    got = _run(tok, tok.decode_streams(3), clips, [_split("eights", 50), _split("random", 50, seed=9), [5] * 10], between=between)
    for k in range(3):
        assert torch.equal(got[k], want[k]), k
    assert one.fed == 36
    solo_out.append(one.feed(solo[:, :, 36:], last=True))
    assert torch.equal(torch.cat(solo_out, dim=2), want_solo)


def test_a_refused_call_consumes_nothing():
    """Each refusal of the header, between two good calls: the corrected call - and the streams' whole output - is bit-equal."""
    tok, full = _tok("voicecraft")
    hop = tok.hop
    clips = [_codes(full, 24, 900), _codes(full, 40, 901), _codes(full, 40, 902)]     # stream 0 ends while the others go on
    want = [tok.decode([(c, None)]) for c in clips]
    st = tok.decode_streams(3)
    out = [[] for _ in range(3)]

    def good(lo, hi, ids=(0, 1, 2), last=()):
        got = st.feed({k: clips[k][:, :, lo:hi] for k in ids}, last=last)
        for k in ids:
            out[k].append(got[k])
    good(0, 16)
    fed, emitted = list(st.fed), list(st.emitted)
    with pytest.raises(AssertionError, match="outside"):
        st.feed({0: clips[0][:, :, 16:24], 3: clips[1][:, :, 16:24]})                 # an id out of range
    with pytest.raises(EngineError, match="capacity"):
        st.feed({0: clips[0][:, :, 16:24], 1: torch.zeros((1, full["n_q"], 400), dtype=torch.int64).cuda()})   # over the capacity
    # (through the C entry point: what the Python wrapper cannot express)
    n = 2
    cd = [clips[k][0, :, 16:24].contiguous() for k in range(2)]
    wav = [torch.empty(8 * hop, device="cuda") for _ in range(2)]
    arr = lambda v: (C.c_int * n)(*v)                                                # noqa: E731
    ptr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])                   # noqa: E731
    got_n = (C.c_int * n)()
    call = tok.lib.vc_codec_decode_streams
    rc = call(tok._h, n, arr([1, 1]), ptr(cd), arr([8, 8]), arr([8, 8]), arr([0, 0]), ptr(wav), arr([8 * hop] * 2), got_n, None)
    assert rc == -1 and b"twice" in tok.lib.vc_codec_last_error(tok._h)
    rc = call(tok._h, n, arr([0, 1]), ptr(cd), arr([8, 8]), arr([8, 8]), arr([0, 0]), ptr(wav), arr([8 * hop, 8 * hop - 1]), got_n, None)
    assert rc == -4 and b"wav capacity" in tok.lib.vc_codec_last_error(tok._h)
    rc = call(tok._h, n, arr([0, 1]), ptr(cd), arr([8, 7]), arr([8, 8]), arr([0, 0]), ptr(wav), arr([8 * hop] * 2), got_n, None)
    assert rc == -1                                                                  # stride < n_frames
    assert st.fed == fed and st.emitted == emitted
    good(16, 24, last=(0,))
    fed, emitted = list(st.fed), list(st.emitted)
    with pytest.raises(EngineError, match="closed"):
        st.feed({0: clips[0][:, :, :4], 1: clips[1][:, :, 24:28]})                    # a closed stream next to an open one
    assert st.fed == fed and st.emitted == emitted
    good(24, 40, ids=(1, 2), last=(1, 2))
    for k in range(3):
        assert torch.equal(torch.cat(out[k], dim=2), want[k]), k
    # more streams than max_batch
    with pytest.raises(AssertionError, match="max_batch"):
        tok.decode_streams(5)
