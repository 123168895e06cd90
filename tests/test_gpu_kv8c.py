"""-m gpu: `kv8="centred"` at engine level (vc_request_kv8c; the contract is in voicecraft_amd/csrc/vc_kv8.h).

1. State after every kind of call: the centres read back lie within one bf16 rounding plus fp32 summation of the mean of the bf16 K rows
   read back (positions 0 .. n0-1, n0 = "kcentre_rows"); the K codes and shifts equal quant.kv8c_quantize_rows(K_bf16, c read back) and
   the V ones quant.kv8_quantize_rows, bit for bit, at every written position; best-of-N siblings and the sequences of a shared-prefix
   call carry the prescribed slot's centre.
2. Teacher-forced logits against the centred test oracle (tests/kv8c_cases.py) within the project's 2e-2 relative L2, with the census.
3. trained_stats A: no kv8, kv8=True and kv8="centred" against the plain fp32 oracle; the centred engine within 2 x the bf16 engine's own.
4. Neutrality: `w8` bit-neutral next to the mode, seeded calls repeat, kv8 = 0 on a centred engine is the bf16 cache bit for bit."""
import numpy as np
import pytest
import torch

import kv8c_cases as cc
import test_gpu_kv8 as t8

pytestmark = pytest.mark.gpu

N_STEPS = t8.N_STEPS


def _engine(preset, kv8="centred", **kw):
    return t8._engine(preset, kv8=kv8, **kw)


def _check_state(eng, n0_want=None, source=None, upto_n0=False):
    """n0_want: {slot: rows of the prefill pass that held its position 0} (exactly these slots hold rows; None: not checked).
    source: {slot: the slot whose centre it must carry} (default: its own, held to the bar).  upto_n0: hold the K codes at positions
    0 .. n0-1 only (a session's slot may keep rows of an earlier request behind the current one's).  Returns n0 per slot."""
    from voicecraft_amd import quant
    a = eng.args
    H, hd = a.nhead, a.d_model // a.nhead
    shape = (eng.max_seqs, H, eng.max_positions, hd)
    n0 = eng.debug_read("kcentre_rows", (eng.max_seqs,), torch.int32).tolist()
    source = source or {}
    found = None
    worst = 0.0
    for l in range(int(a.num_decoder_layers)):
        sh = eng.debug_read(f"kvshift8_{l}", shape[:3] + (2,), torch.int8)
        c = eng.debug_read(f"kcentre_{l}", (eng.max_seqs, H, hd), torch.bfloat16).float()
        k16 = torch.nan_to_num(eng.debug_read(f"kcache{l}", shape, torch.bfloat16).float(), nan=0.0, posinf=0.0, neginf=0.0)
        v16 = torch.nan_to_num(eng.debug_read(f"vcache{l}", shape, torch.bfloat16).float(), nan=0.0, posinf=0.0, neginf=0.0)
        k8, v8 = eng.debug_read(f"kcache8_{l}", shape, torch.uint8), eng.debug_read(f"vcache8_{l}", shape, torch.uint8)
        if found is None:
            found = ((k8 != 0) | (v8 != 0)).any(dim=3).any(dim=1)                 # [slot][position]: the arrays are zeroed at creation
        w = found[:, None, :].expand(shape[:3])
        wk = w
        if upto_n0:
            wk = (torch.arange(shape[2])[None, :] < torch.tensor(n0)[:, None])[:, None, :].expand(shape[:3]) & w
        wc, ws = quant.kv8c_quantize_rows(k16, c)
        assert torch.equal(k8[wk], wc[wk]), (l, "K codes", int((k8[wk] != wc[wk]).sum()))
        assert torch.equal(sh[..., 0][wk], ws[wk]), (l, "K shifts")
        vc_, vs = quant.kv8_quantize_rows(v16)
        assert torch.equal(v8[w], vc_[w]) and torch.equal(sh[..., 1][w], vs[w]), (l, "V")
        for s in range(eng.max_seqs):
            if not bool(found[s].any()):
                continue
            src = source.get(s, s)
            if src != s:
                assert torch.equal(c[s], c[src]) and n0[s] == n0[src], (l, s, "carries the centre of slot", src)
                continue
            assert n0[s] >= 1 and bool(found[s, :n0[s]].all()), (s, n0[s])
            rows = k16[s, :, :n0[s]].double()
            m = rows.mean(dim=1)
            bar = 2.0 ** -8 * m.abs() + 2.0 ** -20 * rows.abs().max()
            err = (c[s].double() - m).abs()
            assert bool((err <= bar).all()), (l, s, float((err / bar).max()))
            worst = max(worst, float((err / bar).max()))
    used = [s for s in range(eng.max_seqs) if bool(found[s].any())]
    if n0_want is not None:
        assert used == sorted(n0_want), (used, sorted(n0_want))
        assert {s: n0[s] for s in used} == n0_want, ({s: n0[s] for s in used}, n0_want)
    return {s: n0[s] for s in used}, worst


def _rows_of(p):
    return p[0].shape[1] + p[2].shape[1] + 1          # text, prompt frames, the first generated column


# ------------------------------------------------------------------------------------------------ 1. state
@pytest.mark.parametrize("preset", ["tiny", "tiny128", "tiny_h16"])
def test_state_after_tts_and_a_two_span_edit(preset):
    from voicecraft_amd import synth
    a, _ = t8._model(preset)
    eng = _engine(preset)
    assert eng.options().endswith("|kv8=1|kv8c=1") and eng.kv8_centred
    p = t8._prompts(a, 1)[0]
    toks = t8._traj(a, N_STEPS, 17)
    c0 = eng.launch_counts()
    eng.inference_tts(p[0].cuda(), p[1].cuda(), p[2].cuda(), top_k=1, stop_repetition=3, _forced=toks, _logit_steps=N_STEPS)
    c = t8._delta(eng.launch_counts(), c0)
    assert c["kv8c_centre"] == 1 and c["kv8c_pack"] == c["kv8_pack"] > 0 and c["kv8c_attn"] == c["kv8_attn"] > 0, c
    _, w1 = _check_state(eng, {0: _rows_of(p)})
    # a second call on the same engine, another prompt: the centre is the new prompt's
    p2 = synth.random_prompt(a, 9, 17, seed=77)
    eng.inference_tts(p2[0].cuda(), p2[1].cuda(), p2[2].cuda(), top_k=1, stop_repetition=3, _forced=toks, _logit_steps=N_STEPS)
    n0, _ = _check_state(eng, upto_n0=True)
    assert n0 == {0: _rows_of(p2)}
    # editing, two spans: the switch between them is a 3-row decode pass
    eng = _engine(preset)
    x, xl, y = synth.random_prompt(a, 6, 30, seed=41)
    spans = [(5, 10), (18, 24)]
    toks = np.concatenate([t8._traj(a, 7, 3, term=a.eog), t8._traj(a, 6, 4, term=a.eog)])
    eng.inference(x.cuda(), xl.cuda(), y.cuda(), torch.tensor([spans]), top_k=1, _forced=toks, _logit_steps=len(toks))
    n0, w2 = _check_state(eng)
    assert list(n0) == [0] and n0[0] >= 6 + (30 - 11), n0
    print(f"\n{preset}: centre bar used {max(w1, w2):.3f}")


@pytest.mark.parametrize("B,max_seqs", [(3, 8), (8, 8), (20, 32)])
def test_state_after_tts_multi(B, max_seqs):
    preset = "tiny128"
    a, _ = t8._model(preset)
    eng = _engine(preset, max_seqs=max_seqs)
    pr = t8._prompts(a, B)
    forced = np.stack([t8._traj(a, N_STEPS, 50 + u) for u in range(B)], axis=1)
    c0 = eng.launch_counts()
    eng.inference_tts_multi([p[0][0] for p in pr], [p[2][0] for p in pr], top_k=1, _forced=forced, _logit_steps=N_STEPS)
    c = t8._delta(eng.launch_counts(), c0)
    assert c["kv8c_centre"] >= 1 and c["kv8c_attn"] > 0, c
    _check_state(eng, {u: _rows_of(pr[u]) for u in range(B)})


@pytest.mark.parametrize("preset", ["tiny", "tiny128", "tiny_h16"])
def test_state_after_best_of_and_a_shared_prefix_call(preset):
    a, _ = t8._model(preset)
    eng = _engine(preset, max_seqs=3)
    p = t8._prompts(a, 1)[0]
    forced = np.stack([t8._traj(a, N_STEPS, 70 + j) for j in range(3)], axis=1)
    eng.inference_tts_batch(p[0].cuda(), p[1].cuda(), p[2].cuda(), top_k=1, batch_size=3, _forced=forced, _logit_steps=N_STEPS)
    _check_state(eng, {0: _rows_of(p), 1: _rows_of(p), 2: _rows_of(p)}, source={1: 0, 2: 0})
    # Long TTS with a shared prefix: the prefix lives in slot 0 only, and every sequence is packed against slot 0's centre
    eng = _engine(preset, max_seqs=3)
    xp = torch.arange(1, 8)
    sents = [torch.arange(10, 10 + 3 + u) for u in range(3)]
    y = p[2]
    eng.inference_tts_long(xp, sents, y, top_k=1, _seed=5)
    n0, _ = _check_state(eng, source={1: 0, 2: 0})
    assert n0 == {s: 7 + 3 + y.shape[1] + 1 for s in range(3)}, n0


def test_state_after_a_session_that_admits_into_used_slots():
    from voicecraft_amd import synth
    preset = "tiny"
    a, _ = t8._model(preset)
    eng = _engine(preset, max_seqs=2)
    eng.set_option("graph_steps", 3)
    pr = [synth.random_prompt(a, 4 + u, 10 + 2 * u, seed=300 + u) for u in range(5)]          # 15, 18, 21, 24, 27 rows
    rows = [_rows_of(p) for p in pr]
    assert len(set(rows)) == 5
    c0 = eng.launch_counts()
    outs = eng.inference_tts_queue([p[0][0] for p in pr], [p[2][0] for p in pr], max_live=2, seeds=[1, 2, 3, 4, 5], top_k=1, stop_repetition=3)
    c = t8._delta(eng.launch_counts(), c0)
    assert len(outs) == 5 and c["kv8c_centre"] >= 3, c
    n0, _ = _check_state(eng, upto_n0=True)
    assert sorted(n0) == [0, 1] and all(v in rows for v in n0.values()), n0
    assert any(v in rows[2:] for v in n0.values()), ("a slot was admitted into again, and holds the later request's centre", n0)


# ------------------------------------------------------------------------------------------------ 2. logits against the centred oracle
@pytest.mark.parametrize("preset,weights", [("tiny", "default"), ("tiny128", "default"), ("tiny_h16", "default"), ("tiny128", "trained_stats_B")])
def test_one_row_tts_logits_against_the_centred_oracle(preset, weights):
    from test_gpu_model import rel_l2
    from voicecraft_amd import synth
    from voicecraft_amd.engine import VoiceCraftEngine
    a, sd = t8._model(preset)
    if weights != "default":
        from oracle.gen_golden import STATS_B
        sd = synth.trained_stats(synth.make_state_dict(a, seed=3, head_gain=4.0), a, **STATS_B)
    prompt = t8._prompts(a, 1, seed=3)[0]
    toks = t8._traj(a, N_STEPS, 17)
    torch.set_num_threads(min(8, torch.get_num_threads()))
    want = cc.centred_tts_logits(cc.Kv8cOracle(a, sd), prompt, toks)
    mk = lambda kv8: VoiceCraftEngine(a, sd, device="cuda:0", dtype="bf16", max_seqs=1, max_positions=256, kv8=kv8)
    eng = mk("centred")
    c0 = eng.launch_counts()
    got = t8._tts_logits(eng, prompt, toks)
    c = t8._delta(eng.launch_counts(), c0)
    assert c["kv8c_centre"] == 1 and c["kv8c_attn"] > 0 and c["kv8c_attn"] == c["kv8_attn"] and c["kv8c_pack"] == c["kv8_pack"] > 0, c
    rel = float(rel_l2(got.reshape(want.shape), want).max())
    eng.set_option("kv8", 0)                               # the same engine on its bf16 cache (it goes on packing)
    assert eng.options().endswith("|kv8=0|kv8c=1")
    c0 = eng.launch_counts()
    off = t8._tts_logits(eng, prompt, toks)
    c = t8._delta(eng.launch_counts(), c0)
    assert c["kv8_attn"] == 0 and c["kv8c_attn"] == 0 and c["kv8c_pack"] > 0, c
    assert np.array_equal(off, t8._tts_logits(mk(False), prompt, toks)), "kv8 = 0 on a centred engine is the bf16 cache, bit for bit"
    with pytest.raises(AssertionError, match="unknown option"):
        eng.set_option("kv8c", 0)                          # the mode is fixed at creation: there is no such option
    print(f"\n{preset} {weights}: centred engine against the centred oracle, worst rel L2 {rel:.2e}")
    assert rel <= 2e-2, rel
    assert np.array_equal(got[0], off[0]) and not np.array_equal(got[1:], off[1:]), "the first step reads no cache"
    assert not np.array_equal(got, t8._tts_logits(mk(True), prompt, toks)), "another grid than kv8=True"


def test_two_span_edit_and_multi_row_logits_against_the_centred_oracle():
    from test_gpu_model import rel_l2
    from voicecraft_amd import synth
    preset = "tiny128"
    a, sd = t8._model(preset)
    torch.set_num_threads(min(8, torch.get_num_threads()))
    orc = cc.Kv8cOracle(a, sd)
    x, xl, y = synth.random_prompt(a, 6, 30, seed=41)
    spans = [(5, 10), (18, 24)]
    toks = np.concatenate([t8._traj(a, 7, 3, term=a.eog), t8._traj(a, 6, 4, term=a.eog)])
    want = cc.centred_edit_logits(orc, x, xl, y, spans, toks)
    _, lg = _engine(preset).inference(x.cuda(), xl.cuda(), y.cuda(), torch.tensor([spans]), top_k=1, _forced=toks, _logit_steps=len(toks))
    rel = float(rel_l2(lg.cpu().numpy().reshape(want.shape), want).max())
    print(f"\n{preset} 2-span edit: centred engine against the centred oracle, worst rel L2 {rel:.2e}")
    assert want.shape[0] == len(toks) and rel <= 2e-2, rel
    B = 8
    pr = t8._prompts(a, B)
    forced = np.stack([t8._traj(a, N_STEPS, 50 + u) for u in range(B)], axis=1)
    _, lg = _engine(preset, max_seqs=8).inference_tts_multi([p[0][0] for p in pr], [p[2][0] for p in pr], top_k=1, _forced=forced, _logit_steps=N_STEPS)
    out = lg.cpu().numpy()
    worst = max(float(rel_l2(out[:, u], cc.centred_tts_logits(orc, pr[u], forced[:, u])).max()) for u in (0, 4, 7))
    print(f"{preset} {B} rows: centred engine against the centred oracle, worst rel L2 {worst:.2e}")
    assert worst <= 2e-2, worst


# ------------------------------------------------------------------------------------------------ 3. trained_stats A
def test_trained_stats_a_three_engines_against_the_plain_oracle():
    """tiny128, trained_stats A, tools/kv8_quality.py's 60 teacher-forced steps against the plain fp32 oracle.  The centred engine's worst
    relative L2 is at most 2 x the no-kv8 bf16 engine's own (the CPU figures: 1.33 x for the round trips alone, 10.8 x for plain kv8)."""
    from voicecraft_amd.engine import VoiceCraftEngine
    a, sd, prompt, want, toks = cc.quality_setup("tiny128", "trained_stats_A")
    fig = {}
    for tag, kv8 in (("bf16", False), ("kv8", True), ("kv8c", "centred")):
        eng = VoiceCraftEngine(a, sd, device="cuda:0", dtype="bf16", max_seqs=1, max_positions=256, kv8=kv8)
        got = t8._tts_logits(eng, prompt, toks)[:cc.STEPS]
        fig[tag] = cc.quality_figures(got.reshape(want.shape), want)
        del eng
    print("\ntiny128 trained_stats_A, engines against the plain fp32 oracle: " + str(fig))
    assert fig["kv8c"]["rel_l2_worst"] <= 2.0 * fig["bf16"]["rel_l2_worst"], fig


# ------------------------------------------------------------------------------------------------ 4. neutrality
def test_w8_stays_bit_neutral_next_to_the_mode():
    preset = "giga330M"
    a, sd = t8._model(preset)
    prompt = t8._prompts(a, 1, seed=3)[0]
    toks = t8._traj(a, N_STEPS, 17)
    e8 = _engine(preset, w8="quantize")
    assert e8.options().endswith("|w8=5|kv8=1|kv8c=1")
    c0 = e8.launch_counts()
    got = t8._tts_logits(e8, prompt, toks)
    c = t8._delta(e8.launch_counts(), c0)
    assert c["w8"] > 0 and c["kv8c_attn"] > 0, c
    from voicecraft_amd.engine import VoiceCraftEngine
    plain = VoiceCraftEngine(a, e8.w8_state_dict, device="cuda:0", dtype="bf16", max_seqs=1, max_positions=256, kv8="centred")
    assert np.array_equal(got, t8._tts_logits(plain, prompt, toks))


def test_seeded_calls_repeat():
    preset = "tiny_h16"
    a, _ = t8._model(preset)
    pr = t8._prompts(a, 4, seed=400)
    runs = []
    for _ in range(2):
        eng = _engine(preset, max_seqs=3)
        x, xl, y = pr[0]
        res = eng.inference_tts(x.cuda(), xl.cuda(), y.cuda(), top_k=40, top_p=1.0, temperature=1.0, stop_repetition=3, _seed=1234)
        outs = eng.inference_tts_queue([p[0][0] for p in pr], [p[2][0] for p in pr], max_live=3, seeds=[11, 12, 13, 14], top_k=40)
        runs.append([res[0].cpu().numpy()] + [o[0].cpu().numpy() for o in outs])
    assert all(p.shape == q.shape and np.array_equal(p, q) for p, q in zip(*runs))


def test_the_request_comes_first_and_is_bf16_only():
    preset = "tiny128"
    a, sd = t8._model(preset)
    eng = _engine(preset, kv8=True)
    assert "kv8c" not in eng.options() and not eng.kv8_centred
    with pytest.raises(AssertionError):
        eng.debug_read("kcentre_0", (16,), torch.bfloat16)
    cen = _engine(preset)
    for bad in ("kcentre_", "kcentre_x", "kcentre_99", "kcentre_0000"):
        with pytest.raises(AssertionError, match="unknown debug buffer"):
            cen.debug_read(bad, (16,), torch.bfloat16)
    assert eng.lib.vc_request_kv8c(eng._h) == -2                       # VC_ESTATE: the request comes before vc_finalize_weights
    assert b"before vc_finalize_weights" in eng.lib.vc_last_error(eng._h)
    from voicecraft_amd.engine import VoiceCraftEngine
    with pytest.raises(AssertionError, match="bf16 engines only"):
        VoiceCraftEngine(a, sd, device="cuda:0", dtype="fp32", max_seqs=1, max_positions=256, kv8="centred")
