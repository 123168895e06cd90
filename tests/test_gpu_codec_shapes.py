"""-m gpu: the HIP EnCodec path over the configurations vc_codec_create accepts, not at the VoiceCraft shape alone.

tests/codec_shapes.py lists the configurations (half, narrow, w768, seq, even, fullsize, seq3) and which kernel form or branch
of vc_codec.hip each one reaches; every test asserts the LSTM / RVQ form the library reports (vc_codec_last_forms).  Per
configuration ONE tokenizer and ONE transformers.EncodecModel restatement on shared synthetic weights:

decode  : T = 1, 3, 40, 130 frames (130 crosses the 128-position tile and the 32-position wave slice of the frame-rate
          convolutions); fullsize: the 101 frames that max_seconds = 2.01 (32160 samples, 100.5 frames) admits.
encode  : clips of 40 hops + 3, 130 hops (fullsize: its full 32160 samples) and hop + 1 samples (two frames: an input shorter
          than the configuration's paddings is zero-extended first); the latent, then the codes.
batches : every item bit-equal to the single-clip call on the same padded row (narrow: 3 clips, half: 2).
LSTM    : persistent launch == wavefront (half), wavefront == step kernels (half, narrow), codes and waveform bit for bit.
stream  : chunks of 1, of 7, everything + an empty final call == the one-shot decode of 40 frames, bit for bit.
RVQ     : exact duplicate codebook rows i < j in another lane group, another wave's tile, a later tile of the same wave and
          the last row: the first maximum wins, no j is ever emitted (narrow, w768, fullsize; fullsize on both searches).

The bars are the project's (tests/test_gpu_codec.py), not re-tuned per shape: latent 1e-3 relative L2, waveform
2e-4 * RMS + 1e-5 max abs, every code disagreement on a near-tie of the oracle's own search at the first stage that differs,
and at most max(1, 1 %) of the (stage, frame) cells disagreeing (clips under 9 frames exempt from the count only).

The floor under each bar, measured on the CPU: the restatement in float32 against itself in float64 (`m.double()`), same
weights (seed 0), same inputs as the tests below - worst case over the lengths of the configuration:

  half     : waveform 0.026 of its bar, latent 8.4e-7 (0.001 of its bar), 0 code cells differ
  narrow   : waveform 0.019 of its bar, latent 6.8e-7 (0.001 of its bar), 0 code cells differ
  w768     : waveform 0.024 of its bar, latent 8.3e-7 (0.001 of its bar), 0 code cells differ
  seq      : waveform 0.012 of its bar, latent 5.9e-7 (0.001 of its bar), 0 code cells differ
  even     : waveform 0.038 of its bar, latent 1.1e-6 (0.001 of its bar), 0 code cells differ
  fullsize : waveform 0.029 of its bar, latent 8.6e-7 (0.001 of its bar), 0 code cells differ
  seq3     : waveform 0.010 of its bar, latent 5.5e-7 (0.001 of its bar), 0 code cells differ
"""
import ctypes as C

import numpy as np
import pytest
import torch

import codec_shapes as cs
from oracle import encodec_oracle as eo
from voicecraft_amd import synth
from voicecraft_amd._lib import EngineError

pytestmark = pytest.mark.gpu

NAMES = list(cs.CONFIGS)
STREAMING = [n for n in NAMES if n != "seq3"]


class Pair:
    """tokenizer + oracle of one configuration, and the oracle's results (computed once, shared, never written to)"""

    def __init__(self, name, max_batch=None):
        from voicecraft_amd.codec import AudioTokenizer
        self.name, self.cfg, self.hop = name, cs.full(name), cs.hop_of(name)
        sd = synth.make_codec_state_dict(cs.SEED[name], cfg=cs.CONFIGS[name])
        self.tok = AudioTokenizer(sd, device="cuda:0", max_seconds=cs.max_seconds(name), cfg=cs.CONFIGS[name],
                                  max_batch=max_batch or cs.MAX_BATCH.get(name, 1))
        self.m = eo.build_cfg(sd, cs.CONFIGS[name])
        self._dec, self._enc = {}, {}

    def oracle_decode(self, T):
        if T not in self._dec:
            self._dec[T] = eo.decode(self.m, cs.random_codes(self.name, T)).numpy()
        return self._dec[T]

    def oracle_encode(self, n):
        if n not in self._enc:
            self._enc[n] = eo.encode(self.m, cs.random_wav(n))
        return self._enc[n]


@pytest.fixture(scope="module")
def pairs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Pair(name)
        return cache[name]
    yield get
    cache.clear()


@pytest.mark.parametrize("name,T", [(n, T) for n in NAMES for T in cs.decode_lengths(n)])
def test_decode_matches_oracle(pairs, name, T):
    pair = pairs(name)
    want = pair.oracle_decode(T)
    got = pair.tok.decode([(cs.random_codes(pair.name, T).unsqueeze(0).cuda(), None)])
    assert got.shape == (1, 1, pair.hop * T)
    got = got[0, 0].cpu().numpy()
    d = float(np.abs(got - want).max())
    print(pair.name, "decode T", T, "max |d|", d, "bar", cs.wave_bar(want))
    assert pair.tok.last_forms()[0] == cs.FORMS[pair.name][0], pair.tok.last_forms()
    assert d <= cs.wave_bar(want), (d, cs.wave_bar(want))


@pytest.mark.parametrize("name,n", [(n, k) for n in NAMES for k in cs.encode_lengths(n)])
def test_encode_matches_oracle(pairs, name, n):
    pair = pairs(name)
    codes_o, z_o = pair.oracle_encode(n)
    out = pair.tok.encode(cs.random_wav(n).cuda())
    codes = out[0][0][0].cpu()
    T = -(-n // pair.hop)
    assert codes.shape == (pair.cfg["n_q"], T) and out[0][1] is None
    assert pair.tok.last_forms() == cs.FORMS[pair.name], pair.tok.last_forms()
    assert codes.min() >= 0 and codes.max() < pair.cfg["codebook_size"]
    z = pair.tok.last_latent(T)
    assert z.shape == z_o.shape
    rel = cs.latent_error(z, z_o)
    print(pair.name, "encode n", n, "latent rel", rel)
    assert rel <= cs.LATENT_BAR, rel
    bad, cells = cs.check_codes(codes, codes_o, z, z_o, cs.oracle_codebooks(pair.m))
    print(pair.name, "encode n", n, "code cells that differ", bad, "of", cells)


def test_full_length_round_trip_when_max_samples_is_no_hop_multiple(pairs):
    """max_seconds = 2.01 is 32160 samples = 100.5 frames: the full clip encodes to 101 frames, and decoding 101 frames
    writes 32320 positions of 64 channels in the last up-sampling stage - the arenas are sized from the frames a call may
    carry, not from max_samples.  The tokenizer's own round trip, then the waveform against the
    oracle's decode of the same codes; one more sample or frame is refused."""
    p = pairs("fullsize")
    tok = p.tok
    assert tok.max_samples == 32160 and tok.max_samples % p.hop
    wav = cs.random_wav(32160)
    codes = tok.encode(wav.cuda())[0][0]
    assert codes.shape == (1, 4, 101)
    back = tok.decode([(codes, None)])
    assert back.shape == (1, 1, 32320) and torch.isfinite(back).all()
    want = eo.decode(p.m, codes[0].cpu()).numpy()
    d = float(np.abs(back[0, 0].cpu().numpy() - want).max())
    assert d <= cs.wave_bar(want), (d, cs.wave_bar(want))
    # the stream's window is held to the same capacity: 101 frames in one chunk, bit for bit the blocking call
    st = tok.decode_stream()
    assert torch.equal(st.feed(codes, last=True), back)
    with pytest.raises(EngineError):
        tok.encode(torch.zeros(1, 1, 32161).cuda())
    with pytest.raises(EngineError):
        tok.decode([(torch.zeros((1, 4, 102), dtype=torch.int64).cuda(), None)])
    st = tok.decode_stream()
    with pytest.raises(EngineError):
        st.feed(torch.zeros((1, 4, 102), dtype=torch.int64).cuda())


@pytest.mark.parametrize("name", ["narrow", "half"])
def test_batch_items_equal_single_calls_bit_for_bit(pairs, name):
    pair = pairs(name)
    tok, hop, B = pair.tok, pair.hop, cs.MAX_BATCH[pair.name]
    assert tok.max_batch == B
    lens = [50 * hop + 5, 31 * hop, 7 * hop + 1][:B]
    g = torch.Generator().manual_seed(3)
    wavs = [torch.randn(n, generator=g) * 0.1 for n in lens]
    padded = torch.nn.utils.rnn.pad_sequence(wavs, batch_first=True).unsqueeze(1)
    codes_b = tok.encode(padded.cuda())[0][0].cpu()
    T = -(-lens[0] // hop)
    assert codes_b.shape == (B, pair.cfg["n_q"], T)
    z_b = torch.empty((B, T, pair.cfg["hidden"]))
    tok._check(tok.lib.vc_codec_debug_latent(tok._h, C.c_void_p(z_b.data_ptr()), z_b.numel()), "latent")
    for b in range(B):
        one = tok.encode(padded[b: b + 1].cuda())[0][0][0].cpu()
        assert torch.equal(one, codes_b[b]), b
        assert torch.equal(tok.last_latent(T), z_b[b]), b
    wav_b = tok.decode([(codes_b.cuda(), None)]).cpu()
    assert wav_b.shape == (B, 1, T * hop)
    for b in range(B):
        assert torch.equal(tok.decode([(codes_b[b: b + 1].cuda(), None)]).cpu()[0], wav_b[b]), b
    # and the first (longest, un-padded) clip is inside the bars against the restatement
    codes_o, z_o = eo.encode(pair.m, padded[:1])
    assert cs.latent_error(z_b[0], z_o) <= cs.LATENT_BAR
    cs.check_codes(codes_b[0], codes_o, z_b[0], z_o, cs.oracle_codebooks(pair.m))


def _round_trip(tok, wav, monkeypatch, env=None):
    for k in ("VC_LSTM_WAVE", "VC_LSTM_SEQUENTIAL"):
        monkeypatch.delenv(k, raising=False)
    if env:
        monkeypatch.setenv(env, "1")
    codes = tok.encode(wav)[0][0]
    enc_form = tok.last_forms()[0]
    back = tok.decode([(codes, None)])
    assert tok.last_forms()[0] == enc_form
    if env:
        monkeypatch.delenv(env)
    return codes, back, enc_form


@pytest.mark.parametrize("name", ["narrow", "half"])
def test_lstm_forms_are_bit_identical(pairs, name, monkeypatch):
    """half (H = 512): the persistent launch == the launch-per-step wavefront (VC_LSTM_WAVE=1).  half and narrow (H = 256, no
    persistent form): the wavefront == the step kernels layer by layer (VC_LSTM_SEQUENTIAL=1), whose upper layer projects
    its input inside the step in the wavefront's order of sums.  Codes AND waveform, a single clip and the whole batch.
    (All three kernels take their dot products and cell update from one helper whose rounding is written out: with the
    compiler choosing the fusions, the step kernels' waveform differed from the wavefront's by 7e-6 at narrow.)"""
    pair = pairs(name)
    tok, hop = pair.tok, pair.hop
    g = torch.Generator().manual_seed(5)
    for B in (1, tok.max_batch):
        wav = (torch.randn(B, 1, 45 * hop + 9, generator=g) * 0.1).cuda()
        codes_w, back_w, form = _round_trip(tok, wav, monkeypatch, "VC_LSTM_WAVE")
        assert form == 1
        codes_d, back_d, form = _round_trip(tok, wav, monkeypatch)
        assert form == cs.FORMS[pair.name][0]                           # half: persistent; narrow: the wavefront again
        assert torch.equal(codes_w, codes_d) and torch.equal(back_w, back_d)
        if B == 1:                                                     # the step kernels take one sequence
            codes_s, back_s, form = _round_trip(tok, wav, monkeypatch, "VC_LSTM_SEQUENTIAL")
            assert form == 0
            assert torch.equal(codes_w, codes_s), float((codes_w != codes_s).float().mean())
            assert torch.equal(back_w, back_s), float((back_w - back_s).abs().max())


SPLITS = {"ones": [1] * 40, "sevens": [7] * 5 + [5], "whole_then_empty": [40, 0]}


@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("name", STREAMING)
def test_stream_equals_the_one_shot_decode_bit_for_bit(pairs, name, split):
    """The configuration's own geometry on the device: every chunk has the promised length, the concatenation is the
    blocking call's waveform."""
    pair = pairs(name)
    tok, hop, T = pair.tok, pair.hop, 40
    codes = cs.random_codes(pair.name, T).unsqueeze(0).cuda()
    want = tok.decode([(codes, None)])
    st = tok.decode_stream()
    sizes, out, fed = SPLITS[split], [], 0
    for i, n in enumerate(sizes):
        last = i == len(sizes) - 1
        before = st.emitted
        w = st.feed(codes[:, :, fed: fed + n], last=last)
        fed += n
        promised = fed * hop if last else st.ready_frames(fed) * hop
        assert w.shape == (1, 1, promised - before), (i, n, w.shape, promised, before)
        out.append(w)
    assert st.closed and st.emitted == T * hop
    got = torch.cat(out, dim=2)
    assert torch.equal(got, want), float((got - want).abs().max())


def _duplicate_rows(name, sd, wav):
    """-> (state dict whose codebooks hold exact duplicates of row 5, the duplicates' indices).  Row 5 of every stage is
    moved onto the mean of that stage's residuals (so that it wins), then copied to rows j > 5 that sit in another lane
    group of the same 16-code tile (9), another wave's tile (21), a later tile of the same wave (69) and the last row."""
    cf = cs.full(name)
    n_codes, i = cf["codebook_size"], 5
    js = sorted({j for j in (9, 21, 69, n_codes - 1) if i < j < n_codes})
    m = eo.build_cfg(sd, cs.CONFIGS[name])
    sd = dict(sd)
    with torch.no_grad():
        r = m.encoder(wav)[0].transpose(0, 1).contiguous()            # [T, hidden]: stage 0 searches the latent itself
        for q in range(cf["n_q"]):
            E = sd[f"quantizer.layers.{q}.codebook.embed"].clone()
            E[i] = r.mean(dim=0)
            for j in js:
                E[j] = E[i]
            sd[f"quantizer.layers.{q}.codebook.embed"] = E
            idx = ((r[:, None, :] - E[None]) ** 2).sum(-1).argmin(dim=1)
            r = r - E[idx]
    return sd, i, js


@pytest.mark.parametrize("name,scalar", [("narrow", False), ("w768", False), ("fullsize", False), ("fullsize", True)])
def test_rvq_first_maximum_wins_among_duplicate_rows(name, scalar, monkeypatch):
    """torch.max returns the FIRST maximum; both searches must.  With rows 5 == j (bit for bit) the two distances are equal
    in every lane, wave and tile that evaluates them, so which of them is emitted is decided by the index comparisons alone:
    in a lane (codes ascend), across the four lane groups and the four waves (rvq_encode_mfma_k's LDS merge: another group
    of the tile, another wave's tile, the last row), across the waves of rvq_encode_k (69 = thread 69, wave 1)."""
    from voicecraft_amd.codec import AudioTokenizer
    hop = cs.hop_of(name)
    wav = cs.random_wav(40 * hop)
    sd, i, js = _duplicate_rows(name, synth.make_codec_state_dict(cs.SEED[name], cfg=cs.CONFIGS[name]), wav)
    assert js and js[-1] == cs.full(name)["codebook_size"] - 1
    m = eo.build_cfg(sd, cs.CONFIGS[name])
    codes_o, z_o = eo.encode(m, wav)
    assert int((codes_o == i).sum()) >= 1, "the oracle's own search never picks the duplicated row at this seed"
    tok = AudioTokenizer(sd, device="cuda:0", max_seconds=41 * hop / cs.SR, cfg=cs.CONFIGS[name], max_batch=1)
    if scalar:
        monkeypatch.setenv("VC_RVQ_SCALAR", "1")
    codes = tok.encode(wav.cuda())[0][0][0].cpu()
    assert tok.last_forms()[1] == (0 if scalar else cs.FORMS[name][1])
    print(name, "scalar" if scalar else "default", "row", i, "emitted", int((codes == i).sum()), "times; oracle", int((codes_o == i).sum()))
    for j in js:
        assert not (codes == j).any(), (j, (codes == j).nonzero()[:4].tolist())
    assert int((codes == i).sum()) >= 1
    z = tok.last_latent(40)
    for j in js:                                                      # the oracle's ties may fall either way: fold them
        codes_o = torch.where(codes_o == j, torch.full_like(codes_o, i), codes_o)
    cs.check_codes(codes, codes_o, z, z_o, cs.oracle_codebooks(m))


@pytest.mark.parametrize("name", ["w768", "narrow"])
def test_a_code_index_past_a_small_codebook_is_refused(pairs, name):
    """C = 8 and C = 16: an index >= C, in the blocking call and in the stream; the codec stays usable."""
    pair = pairs(name)
    tok, cf = pair.tok, pair.cfg
    bad = cs.random_codes(name, 6).unsqueeze(0)
    bad[0, cf["n_q"] - 1, 4] = cf["codebook_size"]
    with pytest.raises(AssertionError, match="code index outside"):
        tok.decode([(bad.cuda(), None)])
    st = tok.decode_stream()
    with pytest.raises(AssertionError, match="code index outside"):
        st.feed(bad.cuda(), last=True)
    got = tok.decode([(cs.random_codes(name, 3).unsqueeze(0).cuda(), None)])[0, 0].cpu().numpy()
    assert np.abs(got - pair.oracle_decode(3)).max() <= cs.wave_bar(pair.oracle_decode(3))


def test_three_lstm_layers_have_no_stream_and_say_so(pairs):
    tok = pairs("seq3").tok
    with pytest.raises(AssertionError, match="at most 2 LSTM layers"):
        tok.decode_stream()
    T = 3                                                             # the blocking calls are untouched by the refusal
    got = tok.decode([(cs.random_codes("seq3", T).unsqueeze(0).cuda(), None)])[0, 0].cpu().numpy()
    assert np.abs(got - pairs("seq3").oracle_decode(T)).max() <= cs.wave_bar(pairs("seq3").oracle_decode(T))


def test_a_batched_call_without_the_two_layer_wavefront_is_refused(pairs):
    """seq: one LSTM layer at H = 128 runs on the step kernels, which take one sequence."""
    p2 = Pair("seq", max_batch=2)
    wav = cs.random_wav(20 * p2.hop, B=2).cuda()
    with pytest.raises(AssertionError, match="batched LSTM needs the two-layer wavefront"):
        p2.tok.encode(wav)
    with pytest.raises(AssertionError, match="batched LSTM needs the two-layer wavefront"):
        p2.tok.decode([(torch.stack([cs.random_codes("seq", 20)] * 2).cuda(), None)])
    one = p2.tok.encode(wav[:1])[0][0]                               # single clips still run, and equal the other tokenizer's
    assert torch.equal(one, pairs("seq").tok.encode(wav[:1])[0][0])
