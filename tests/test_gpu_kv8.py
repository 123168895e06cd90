"""-m gpu: option `kv8` at engine level - a bf16 engine created with `kv8=True` keeps an E4M3 copy of every layer's K / V cache
(kv8_pack_k behind every pass) and its decode passes read the positions older than the pass from it (rows_attn_k, kv8 form).

1. Cache equality, exact: after every kind of call, at every written position of every used slot, the E4M3 bytes and shifts equal
   quant.kv8_quantize_rows of the bf16 rows.  "Written" is read off the E4M3 K cache itself (it is zeroed at creation; a written K row
   of all heads is never all zeros), and the test pins how many slots and positions each call must have written.
2. Teacher-forced logits against the kv8 test oracle (tests/kv8_cases.py) within the project's bf16 bar of 2e-2 relative L2, different
   from the engine without kv8, with the census counters.
3. `w8` stays bit-neutral next to it.  4. Determinism.  5. An engine without the request is unchanged."""
import functools

import numpy as np
import pytest
import torch

import kv8_cases as kc

pytestmark = pytest.mark.gpu

N_STEPS = 12
GIGA_LAYERS = {"giga330M": 2, "giga830M": 1}


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


@functools.lru_cache(maxsize=None)
def _model(preset):
    from voicecraft_amd import synth
    kw = {"num_decoder_layers": GIGA_LAYERS[preset]} if preset in GIGA_LAYERS else {}
    a = synth.make_args(preset, **kw)
    return a, synth.make_state_dict(a, seed=0, fast=True)


def _traj(a, n, seed, term=None):
    K = a.n_codebooks
    toks = np.random.RandomState(seed).randint(0, a.audio_vocab_size, size=(n, K)).astype(np.int64)
    for j in range(K):
        toks[n - K + j, :j] = a.empty_token
        toks[n - K + j, j] = a.eos if term is None else term
    return toks


def _engine(preset, kv8=True, max_seqs=1, max_positions=256, **kw):
    from voicecraft_amd.engine import VoiceCraftEngine
    a, sd = _model(preset)
    return VoiceCraftEngine(a, sd, device="cuda:0", dtype="bf16", max_seqs=max_seqs, max_positions=max_positions, kv8=kv8, **kw)


def _prompts(a, n, seed=100):
    from voicecraft_amd import synth
    return [synth.random_prompt(a, 4 + (3 * u) % 7, 10 + (5 * u) % 9, seed=seed + u) for u in range(n)]


def _check_caches(eng, min_written=None):
    """min_written: {slot: (first position, positions)} the call must have written at least, in exactly these slots (None: not checked).
    Returns {slot: (first position, positions)} found."""
    from voicecraft_amd import quant
    a = eng.args
    H, hd = a.nhead, a.d_model // a.nhead
    shape = (eng.max_seqs, H, eng.max_positions, hd)
    found = None
    for l in range(int(a.num_decoder_layers)):
        sh = eng.debug_read(f"kvshift8_{l}", shape[:3] + (2,), torch.int8)
        for j, n in enumerate("kv"):
            c16 = eng.debug_read(f"{n}cache{l}", shape, torch.bfloat16).float()
            c8 = eng.debug_read(f"{n}cache8_{l}", shape, torch.uint8)
            if found is None:
                found = (c8 != 0).any(dim=3).any(dim=1)                     # [slot][position]
            w = found[:, None, :].expand(shape[:3])
            rows = torch.nan_to_num(c16[w], nan=0.0, posinf=0.0, neginf=0.0)      # (written rows are finite: asserted through equality below)
            assert bool(torch.isfinite(c16[w]).all()), (l, n)
            wc, ws = quant.kv8_quantize_rows(rows)
            assert torch.equal(c8[w], wc), (l, n, int((c8[w] != wc).sum()))
            assert torch.equal(sh[..., j][w], ws), (l, n)
    got = {}
    for s in range(eng.max_seqs):
        p = torch.nonzero(found[s]).reshape(-1).tolist()
        if p:
            assert p == list(range(p[0], p[-1] + 1)), (s, "written positions are one run")
            got[s] = (p[0], len(p))
    if min_written is not None:
        for s, (p0, n) in min_written.items():
            assert s in got and got[s][0] == p0 and got[s][1] >= n, (s, got.get(s), (p0, n))
        assert set(got) == set(min_written), (sorted(got), sorted(min_written))
    return got


# ------------------------------------------------------------------------------------------------ 1. cache equality
@pytest.mark.parametrize("preset", ["tiny", "tiny128", "tiny_h16"])
def test_cache_equality_tts_and_two_span_edit(preset):
    a, _ = _model(preset)
    eng = _engine(preset)
    x, xl, y = _prompts(a, 1)[0]
    toks = _traj(a, N_STEPS, 17)
    c0 = eng.launch_counts()
    eng.inference_tts(x.cuda(), xl.cuda(), y.cuda(), top_k=1, stop_repetition=3, _forced=toks, _logit_steps=N_STEPS)
    c = _delta(eng.launch_counts(), c0)
    assert c["kv8_pack"] > 0 and c["kv8_attn"] > 0 and c["kv8_attn"] <= c["rows_attn"], c
    Lx, T = x.shape[1], y.shape[1]
    _check_caches(eng, {0: (0, Lx + T + 1 + N_STEPS - a.n_codebooks)})      # the prompt's rows and a row per step in front of the staggered end
    # editing, two spans: the switch between them is a 3-row decode pass
    del eng
    eng = _engine(preset)
    from voicecraft_amd import synth
    x, xl, y = synth.random_prompt(a, 6, 30, seed=41)
    spans = [(5, 10), (18, 24)]
    toks = np.concatenate([_traj(a, 7, 3, term=a.eog), _traj(a, 6, 4, term=a.eog)])
    eng.inference(x.cuda(), xl.cuda(), y.cuda(), torch.tensor([spans]), top_k=1, _forced=toks, _logit_steps=len(toks))
    _check_caches(eng, {0: (0, 6 + (30 - 11) + len(toks) - 2 * a.n_codebooks)})      # text, kept frames, the plain steps of both spans


@pytest.mark.parametrize("B,max_seqs", [(3, 8), (8, 8), (20, 33), (33, 33)])
def test_cache_equality_tts_multi(B, max_seqs):
    """3 and 8 rows: finished-row forms (split and unsplit attention); 20 and 33: wide steps (x_out form)."""
    preset = "tiny128"
    a, _ = _model(preset)
    eng = _engine(preset, max_seqs=max_seqs)
    pr = _prompts(a, B)
    forced = np.stack([_traj(a, N_STEPS, 50 + u) for u in range(B)], axis=1)
    c0 = eng.launch_counts()
    eng.inference_tts_multi([p[0][0] for p in pr], [p[2][0] for p in pr], top_k=1, _forced=forced, _logit_steps=N_STEPS)
    c = _delta(eng.launch_counts(), c0)
    assert c["kv8_attn"] > 0 and c["kv8_pack"] > 0, c
    _check_caches(eng, {u: (0, pr[u][0].shape[1] + pr[u][2].shape[1] + 1 + N_STEPS - a.n_codebooks) for u in range(B)})


def test_cache_equality_edit_multi_best_of_and_long():
    from voicecraft_amd import synth
    preset = "tiny"
    a, _ = _model(preset)
    eng = _engine(preset, max_seqs=6)
    reqs = []
    for u, spans in enumerate([[(4, 8), (12, 15)], [(5, 9)], [(3, 4), (10, 14)]]):
        x, _, y = synth.random_prompt(a, 4 + u, 24 + u, seed=950 + u)
        reqs.append((x, y, spans))
    eng.inference_multi([r[0][0] for r in reqs], [r[1][0] for r in reqs], [r[2] for r in reqs], top_k=1, stop_repetition=-1)
    got = _check_caches(eng, {u: (0, 20) for u in range(3)})
    assert all(n > 25 for _, n in got.values()), got
    # best-of-3: the siblings' rows are copies of the first sample's prompt rows, then their own steps
    eng = _engine(preset, max_seqs=3)
    x, xl, y = _prompts(a, 1)[0]
    forced = np.stack([_traj(a, N_STEPS, 70 + j) for j in range(3)], axis=1)
    eng.inference_tts_batch(x.cuda(), xl.cuda(), y.cuda(), top_k=1, batch_size=3, _forced=forced, _logit_steps=N_STEPS)
    n = x.shape[1] + y.shape[1] + 1 + N_STEPS - a.n_codebooks
    _check_caches(eng, {0: (0, n), 1: (0, n), 2: (0, n)})
    # Long TTS with a shared prefix: the prefix lives in slot 0 only
    eng = _engine(preset, max_seqs=3)
    xp = torch.arange(1, 8)
    sents = [torch.arange(10, 10 + 3 + u) for u in range(3)]
    y = _prompts(a, 1)[0][2]
    eng.inference_tts_long(xp, sents, y, top_k=1, _seed=5)
    got = _check_caches(eng, {0: (0, 7 + 3 + y.shape[1] + 2), 1: (7, 4 + y.shape[1] + 2), 2: (7, 5 + y.shape[1] + 2)})
    assert all(n > 20 for _, n in got.values()), got


def test_cache_equality_session_with_admissions_best_of_and_cancel():
    preset = "tiny"
    a, _ = _model(preset)
    eng = _engine(preset, max_seqs=4)
    eng.set_option("graph_steps", 3)
    pr = _prompts(a, 5, seed=300)
    with eng.open_session(4, top_k=1, stop_repetition=3, max_samples=2) as sess:
        t = [sess.submit(*pr[0], seed=1), sess.submit(*pr[1], seed=2, n_samples=2)]
        done = {}
        for _ in range(3):
            done.update({k: r for k, r, g in sess.poll()})
        t += [sess.submit(*pr[2], seed=3), sess.submit(*pr[3], seed=4), sess.submit(*pr[4], seed=5)]      # admitted as slots free up
        for _ in range(2):
            done.update({k: r for k, r, g in sess.poll()})
        if t[0] not in done:
            assert sess.cancel(t[0]) in ("live", "finished")
        done.update({k: r for k, r, g in sess.drain()})
        assert set(done) >= set(t[1:])
    got = _check_caches(eng)
    assert sorted(got) == [0, 1, 2, 3] and all(p0 == 0 and n > 15 for p0, n in got.values()), got      # every slot of the session was used


# ------------------------------------------------------------------------------------------------ 2. logits against the kv8 oracle
def _tts_logits(eng, prompt, toks):
    x, xl, y = prompt
    _, _, lg = eng.inference_tts(x.cuda(), xl.cuda(), y.cuda(), top_k=1, stop_repetition=3, _forced=toks, _logit_steps=len(toks))
    return lg.cpu().numpy()


@pytest.mark.parametrize("preset", ["tiny", "tiny128", "tiny_h16", "giga330M", "giga830M"])
def test_one_row_tts_logits_against_the_kv8_oracle(preset):
    from test_gpu_model import rel_l2
    a, sd = _model(preset)
    prompt = _prompts(a, 1, seed=3)[0]
    toks = _traj(a, N_STEPS, 17)
    torch.set_num_threads(min(8, torch.get_num_threads()))
    want = kc.cached_tts_logits(kc.Kv8Oracle(a, sd), prompt, toks)
    eng = _engine(preset)
    assert eng.options().endswith("|kv8=1")
    c0 = eng.launch_counts()
    got = _tts_logits(eng, prompt, toks)
    c = _delta(eng.launch_counts(), c0)
    assert c["kv8_attn"] > 0 and c["kv8_pack"] > 0, c
    rel = float(rel_l2(got.reshape(want.shape), want).max())
    eng.set_option("kv8", 0)                               # the same engine on its bf16 cache (it goes on packing)
    assert eng.options().endswith("|kv8=0")
    c0 = eng.launch_counts()
    off = _tts_logits(eng, prompt, toks)
    c = _delta(eng.launch_counts(), c0)
    assert c["kv8_attn"] == 0 and c["kv8_pack"] > 0, c
    plain = _tts_logits(_engine(preset, kv8=False), prompt, toks)
    assert np.array_equal(off, plain), "kv8 = 0 is the engine without the option"
    rel_off = float(rel_l2(off.reshape(want.shape), want).max())
    print(f"\n{preset}: kv8 engine against the kv8 oracle, worst rel L2 {rel:.2e}; the bf16 cache against the same oracle {rel_off:.2e}")
    assert rel <= 2e-2, rel
    assert np.array_equal(got[0], off[0]) and not np.array_equal(got[1:], off[1:]), "the first step reads no cache, every later one the E4M3 one"


def test_two_span_edit_logits_against_the_kv8_oracle():
    from test_gpu_model import rel_l2
    from voicecraft_amd import synth
    preset = "tiny128"
    a, sd = _model(preset)
    x, xl, y = synth.random_prompt(a, 6, 30, seed=41)
    spans = [(5, 10), (18, 24)]
    toks = np.concatenate([_traj(a, 7, 3, term=a.eog), _traj(a, 6, 4, term=a.eog)])
    torch.set_num_threads(min(8, torch.get_num_threads()))
    want = kc.cached_edit_logits(kc.Kv8Oracle(a, sd), x, xl, y, spans, toks)
    out = {}
    for kv8 in (True, False):
        eng = _engine(preset, kv8=kv8)
        _, lg = eng.inference(x.cuda(), xl.cuda(), y.cuda(), torch.tensor([spans]), top_k=1, _forced=toks, _logit_steps=len(toks))
        out[kv8] = lg.cpu().numpy()
    rel = float(rel_l2(out[True].reshape(want.shape), want).max())
    print(f"\n{preset} 2-span edit: kv8 engine against the kv8 oracle, worst rel L2 {rel:.2e}")
    assert want.shape[0] == len(toks) and rel <= 2e-2, rel
    assert not np.array_equal(out[True], out[False])


@pytest.mark.parametrize("B,max_seqs", [(3, 8), (8, 8), (20, 32)])
def test_multi_row_tts_logits_against_the_kv8_oracle(B, max_seqs):
    from test_gpu_model import rel_l2
    preset = "tiny128"
    a, sd = _model(preset)
    pr = _prompts(a, B)
    forced = np.stack([_traj(a, N_STEPS, 50 + u) for u in range(B)], axis=1)
    out = {}
    for kv8 in (True, False):
        eng = _engine(preset, kv8=kv8, max_seqs=max_seqs)
        c0 = eng.launch_counts()
        _, lg = eng.inference_tts_multi([p[0][0] for p in pr], [p[2][0] for p in pr], top_k=1, _forced=forced, _logit_steps=N_STEPS)
        c = _delta(eng.launch_counts(), c0)
        assert (c["kv8_attn"] > 0) == kv8 and (c["kv8_pack"] > 0) == kv8, c
        out[kv8] = lg.cpu().numpy()
    torch.set_num_threads(min(8, torch.get_num_threads()))
    orc = kc.Kv8Oracle(a, sd)
    worst = 0.0
    for u in sorted({0, B // 2, B - 1}):
        want = kc.cached_tts_logits(orc, pr[u], forced[:, u])
        worst = max(worst, float(rel_l2(out[True][:, u], want).max()))
    print(f"\n{preset} {B} rows: kv8 engine against the kv8 oracle, worst rel L2 {worst:.2e}")
    assert worst <= 2e-2, worst
    assert not np.array_equal(out[True], out[False])


# ------------------------------------------------------------------------------------------------ 3. w8, 4. determinism, 5. no request
def test_w8_stays_bit_neutral_next_to_kv8():
    preset = "giga330M"
    a, sd = _model(preset)
    prompt = _prompts(a, 1, seed=3)[0]
    toks = _traj(a, N_STEPS, 17)
    e8 = _engine(preset, w8="quantize")
    assert e8.options().endswith("|w8=5|kv8=1")
    c0 = e8.launch_counts()
    got = _tts_logits(e8, prompt, toks)
    c = _delta(e8.launch_counts(), c0)
    assert c["w8"] > 0 and c["kv8_attn"] > 0, c
    from voicecraft_amd.engine import VoiceCraftEngine
    plain = VoiceCraftEngine(a, e8.w8_state_dict, device="cuda:0", dtype="bf16", max_seqs=1, max_positions=256, kv8=True)
    assert np.array_equal(got, _tts_logits(plain, prompt, toks))


def test_determinism_of_a_seeded_call_and_a_session_schedule():
    preset = "tiny_h16"
    a, _ = _model(preset)
    pr = _prompts(a, 4, seed=400)
    runs = []
    for _ in range(2):
        eng = _engine(preset, max_seqs=3)
        x, xl, y = pr[0]
        res = eng.inference_tts(x.cuda(), xl.cuda(), y.cuda(), top_k=40, top_p=1.0, temperature=1.0, stop_repetition=3, _seed=1234)
        outs = eng.inference_tts_queue([p[0][0] for p in pr], [p[2][0] for p in pr], max_live=3, seeds=[11, 12, 13, 14], top_k=40)
        runs.append([res[0].cpu().numpy()] + [o[0].cpu().numpy() for o in outs])
    assert all(p.shape == q.shape and np.array_equal(p, q) for p, q in zip(*runs))
    assert runs[0][0].shape[-1] > pr[0][2].shape[1] + 4


def test_engine_without_the_request_is_unchanged():
    preset = "tiny128"
    a, sd = _model(preset)
    eng = _engine(preset, kv8=False)
    assert eng.options().endswith("|w13=5") and "kv8" not in eng.options()
    with pytest.raises(AssertionError, match="vc_request_kv8"):
        eng.set_option("kv8", 1)
    for name in ("kcache8_0", "vcache8_0", "kvshift8_0"):
        with pytest.raises(AssertionError):
            eng.debug_read(name, (16,), torch.uint8)
    c0 = eng.launch_counts()
    _tts_logits(eng, _prompts(a, 1, seed=3)[0], _traj(a, N_STEPS, 17))
    c = _delta(eng.launch_counts(), c0)
    assert c["kv8_attn"] == 0 and c["kv8_pack"] == 0 and c["rows_attn"] > 0, c
    assert eng.lib.vc_request_kv8(eng._h) == -2                        # VC_ESTATE: the request comes before vc_finalize_weights
    assert b"before vc_finalize_weights" in eng.lib.vc_last_error(eng._h)
    from voicecraft_amd.engine import VoiceCraftEngine
    with pytest.raises(AssertionError, match="bf16 engines only"):
        VoiceCraftEngine(a, sd, device="cuda:0", dtype="fp32", max_seqs=1, max_positions=256, kv8=True)
