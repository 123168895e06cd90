"""-m gpu: the shared text prefix of sentence-chained calls (vc_tts_multi shared_text_prefix = P) on every attention path
that implements the redirect "positions < P come from sequence 0's cache" - tile_attn_k (wave-uniform fast path on either side of
the boundary, per-lane path in the tile that straddles it), tile_attn64_k, multi-pass prefill, rows_attn_k's general form in every
decode form (8 / 4 / 2 splits with bf16 and fp32 partials, unsplit, wide, the refill loop), retirement of sequence 0, the best-of-N
sibling copy - with P at the tile edges of both compute dtypes (tests/shared_prefix_cases.py holds the table).

Per case, on ONE engine: (1) a stale call of the same shapes on other text, so that every slot's own cache holds foreign K/V below P;
(2) the call with the prefix shared; (3) the same call without sharing.  (2) and (3) are teacher-forced on the same tokens.
  (a) differential: rel L2 of (2) against (3), per slot and step, <= defect_floor(case) / 4 - the floor is the distance the MILDEST
      modelled fault (a boundary off by one row) puts between the oracle's own logits, so a correct engine sits four times closer to
      its own result without reuse than any such fault would put it; the bound comes from the oracle alone
  (b) (2) against an independent oracle call on each full text at the project's bars (bf16: rel L2 <= 2e-2; fp32: 1e-3 absolute, same arg-max)
  (c) the launch census of (2) shows the kernel form the case is listed for
  (d) a later plain inference_tts on the same engine equals a fresh engine's: the share word was cleared.
The measured distances are printed per case (pytest -s; profiles/shared_prefix_pytest_gpu.log)."""
import functools

import numpy as np
import pytest
import torch

import shared_prefix_cases as sp

pytestmark = pytest.mark.gpu


def _engine(c, max_positions=256):
    from voicecraft_amd.engine import VoiceCraftEngine
    a, sd = sp.model(c.preset)
    eng = VoiceCraftEngine(a, sd, device="cuda:0", dtype=c.dtype, max_seqs=max(2, c.slots), max_positions=max_positions)
    for k, v in c.options:
        eng.set_option(k, v)
    return eng


def _plain_inputs(preset):
    """A plain one-utterance call for (d): 23 prompt rows, one row per step - launch forms that no case's options change."""
    from voicecraft_amd import synth
    a, _ = sp.model(preset)
    x, xl, y = synth.random_prompt(a, 7, 15, seed=41)
    K, n = a.n_codebooks, 8
    toks = np.random.RandomState(43).randint(0, a.audio_vocab_size, size=(n, K)).astype(np.int64)
    for j in range(K):
        toks[n - K + j, :j] = a.empty_token
        toks[n - K + j, j] = a.eos
    return x, xl, y, toks


def _plain_call(eng, preset):
    x, xl, y, toks = _plain_inputs(preset)
    res, _, lg = eng.inference_tts(x.cuda(), xl.cuda(), y.cuda(), top_k=1, stop_repetition=3, _forced=toks, _logit_steps=len(toks))
    return res.cpu().numpy(), lg.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _fresh_plain(preset, dtype, options):
    """The plain call on an engine that never shared a prefix (same options as the case's engine)."""
    return _plain_call(_engine(sp.Case("fresh", "", preset, dtype, 0, (1,), options=options)), preset)


def _call(eng, c, texts, y, forced, share):
    n = max(c.n_steps(s, forced.shape[2]) for s in range(c.slots))
    outs, lg = eng.inference_tts_multi(texts, [y] * c.B, top_k=1, stop_repetition=3, _forced=forced, _logit_steps=n,
                                       _shared_text_prefix=share, batch_size=c.N)
    assert len(outs) == c.B
    return lg.cpu().numpy()                     # [steps, slots, K, V]


@pytest.mark.parametrize("name", [c.name for c in sp.CASES])
def test_shared_prefix_case(name, capsys):
    c = sp.BY_NAME[name]
    a, _ = sp.model(c.preset)
    K = a.n_codebooks
    texts, stale, y, y_stale, forced = sp.inputs(name)
    ref = sp.reference(name)
    floor = sp.defect_floor(c)
    assert floor >= sp.FLOOR_MIN
    eng = _engine(c)
    c00 = eng.launch_counts()
    _call(eng, c, stale, y_stale, forced, 0)                                  # (1)
    c0 = eng.launch_counts()
    reuse = _call(eng, c, texts, y, forced, c.P)                              # (2)
    c1 = eng.launch_counts()
    # the prefill launches of (2) alone; the decode steps' launches are counted when their graph is captured, which the first call of
    # a shape does - (1), whose graphs (2) replays with the share word set: those slots are taken over both calls
    census = {k: v - (c00[k] if k in ("rows_attn", "wd") else c0[k]) for k, v in c1.items()}
    plain = _call(eng, c, texts, y, forced, 0)                                # (3)
    later = _plain_call(eng, c.preset)
    dist, orc = {}, {}
    for s in range(c.slots):
        n = c.n_steps(s, K)
        dist[s] = sp.rel_l2(reuse[:n, s], plain[:n, s])
        want = ref["clean"][s]
        orc[s] = sp.rel_l2(reuse[:n, s], want) if c.dtype == "bf16" else np.abs(reuse[:n, s] - want).max(axis=(1, 2))
    worst = max(float(d.max()) for d in dist.values())
    with capsys.disabled():
        print(f"\n[shared-prefix] {name}: context {c.context} floor {floor:.3e} bound {floor / 4:.3e} measured reuse-vs-plain max {worst:.3e} "
              f"(per slot {' '.join(f'{float(d.max()):.1e}' for d in dist.values())}); oracle "
              f"{'rel L2' if c.dtype == 'bf16' else 'max abs'} max {max(float(o.max()) for o in orc.values()):.3e}")
    # (c) the census first: a case that runs another form than it is listed for proves nothing
    for slot, wanted in c.census:
        assert (census[slot] > 0) == wanted, (slot, census)
    # (a)
    for s, d in dist.items():
        assert np.isfinite(d).all() and d.max() <= floor / 4, (s, d.tolist(), floor / 4)
    # (b)
    for s, o in orc.items():
        n = c.n_steps(s, K)
        if c.dtype == "bf16":
            assert o.max() <= 2e-2, (s, o.tolist())
        else:
            assert o.max() <= 1e-3, (s, o.tolist())
            assert np.array_equal(reuse[:n, s].argmax(-1), ref["clean"][s].argmax(-1)), s
    # (d)
    fresh = _fresh_plain(c.preset, c.dtype, c.options)
    assert np.array_equal(later[0], fresh[0]) and np.array_equal(later[1], fresh[1]), float(np.abs(later[1] - fresh[1]).max())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_prefix_longer_than_the_check_kernels_workgroup_is_verified_to_its_last_token(dtype):
    """prompt_k compares the claimed prefix in a strided loop of one workgroup: with P = 300 (more than its threads) a text that differs
    from sequence 0's at index 299 is refused, one that differs first at index 300 runs."""
    from voicecraft_amd import synth
    from voicecraft_amd.engine import VoiceCraftEngine
    a, sd = sp.model("tiny")
    P = 300
    rs = np.random.RandomState(3)
    x0 = torch.from_numpy(rs.randint(0, a.text_vocab_size, size=P + 4).astype(np.int64))
    _, _, y = synth.random_prompt(a, 1, 6, seed=2)
    K = a.n_codebooks
    toks = rs.randint(0, a.audio_vocab_size, size=(1 + K, 2, K)).astype(np.int64)
    for j in range(K):                      # both sequences end at once: the call is five steps long
        toks[1 + j, :, :j] = a.empty_token
        toks[1 + j, :, j] = a.eos
    eng = VoiceCraftEngine(a, sd, device="cuda:0", dtype=dtype, max_seqs=2, max_positions=512)
    for idx, ok in ((299, False), (300, True), (0, False), (255, False), (256, False)):
        x1 = torch.cat([x0, x0[:3]])
        x1[idx] = (x1[idx] + 1) % a.text_vocab_size
        if ok:
            outs = eng.inference_tts_multi([x0, x1], [y[0], y[0]], top_k=1, _forced=toks, _shared_text_prefix=P)
            assert len(outs) == 2
        else:
            with pytest.raises(AssertionError, match="shared_text_prefix"):
                eng.inference_tts_multi([x0, x1], [y[0], y[0]], top_k=1, _forced=toks, _shared_text_prefix=P)
