"""-m gpu: parity in the VALUE regime of a trained checkpoint (tests/trained_stats_cases.py, `synth.trained_stats`).

Every other parity test runs on default-initialised weights: residual rows with |mean| << sigma and a nearly uniform softmax.  There
the kernels' centring before a bf16 rounding (PRO_LN / PRO_LNW / the producers' centred copy behind PRO_LNQ / ln_rows_k), the
`E[q^2] - mean(q)^2` epilogues and every correction factor of the online softmax (FAST and per-visit forms of rows_attn_k, the 8-wave
LDS merge, the split merge in the out-projection, tile_attn_k / tile_attn64_k) could be wrong without a test noticing.  Here: setting
A (common offset 32 per embedding that drifts by 4 per residual update, q/k gain 3, key bias 40 in fp32 / 8 in bf16: raw scores beyond
+-88.7) and setting B (four massive-activation channels carry a row's sigma).  tests/test_trained_stats_cpu.py checks on the oracle
alone that the inputs are in that regime and that the fp32 oracle decides every greedy token with a margin >= 100 x its own rounding.

fp32: FREE-running greedy tokens equal the oracle's and every step's head logits are within 1e-3.  bf16: teacher-forced on the oracle's
trajectory, per-step relative L2 <= 2e-2 for every sequence.  Every test asserts the kernel form it means to cover from the
launch census (eager loops: every launch is counted) or vc_debug_plan."""
import ctypes as C

import numpy as np
import pytest
import torch

import trained_stats_cases as tc
from test_gpu_model import rel_l2

pytestmark = pytest.mark.gpu


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


def _plan(a, dtype, rows):
    from voicecraft_amd import _lib
    from voicecraft_amd._lib import ModelCfg
    av = a.audio_vocab_size
    cfg = ModelCfg(d_model=a.d_model, nhead=a.nhead, num_layers=a.num_decoder_layers, n_codebooks=a.n_codebooks, audio_vocab_size=av,
                   n_special=4, text_rows=101, head_hidden=av // 2, empty_token=av, eog=av + 1, audio_pad_token=av + 2, eos=av + 3,
                   reduced_eog=1, encodec_sr=50, max_n_spans=3, max_seqs=64, max_positions=1024)
    out = (C.c_int32 * 16)()
    assert _lib.load().vc_debug_plan(C.byref(cfg), _lib.VC_DTYPE_BF16 if dtype == "bf16" else _lib.VC_DTYPE_F32, rows, out) == 0
    return list(out)      # [frmax, form, nsplit, mt, oform, dform, heads_lnw, even, fr1, qkv_p8, frp, wd, ...] (tests/test_plan_cpu.py)


def _engine(a, sd, dtype, B, graph=False, max_positions=256):
    from voicecraft_amd.engine import VoiceCraftEngine
    return VoiceCraftEngine(a, sd, device="cuda:0", dtype=dtype, max_seqs=B, max_positions=max_positions, use_graph=graph)


def _worst_abs(got, want):
    live = np.abs(want) < 1e3
    return float(np.abs((got - want) * live).max())


def _batch(preset, key, B):
    """Sequences 0..B-1 of the ragged family with their oracle runs, and the forced-token array of a teacher-forced call."""
    runs = [tc.tts_run(preset, key, u) for u in range(B)]
    n = max(len(r[3]) for r in runs)
    forced = np.zeros((n, B, runs[0][3].shape[1]), dtype=np.int64)
    for b, r in enumerate(runs):
        forced[: len(r[3]), b] = r[3]
    return runs, forced, n


def _multi(eng, runs, forced=None, n=0):
    xs, ys = [r[0][0][0] for r in runs], [r[0][2][0] for r in runs]
    if forced is None:
        return eng.inference_tts_multi(xs, ys, **tc.KNOBS, _logit_steps=n)
    return eng.inference_tts_multi(xs, ys, **tc.KNOBS, _forced=forced, _logit_steps=n)


def _check_multi_fp32(runs, outs, lg, tag):
    lg = lg.cpu().numpy()
    worst = 0.0
    for b, r in enumerate(runs):
        assert np.array_equal(outs[b][0].cpu().numpy(), r[1]), (tag, b)
        worst = max(worst, _worst_abs(lg[: len(r[2]), b], r[2]))
    print(f"fp32 {tag}: worst |d| {worst:.2e}")
    assert worst <= 1e-3, (tag, worst)
    return worst


def _check_multi_bf16(runs, lg, tag):
    lg = lg.cpu().numpy()
    worst = max(float(rel_l2(lg[: len(r[2]), b], r[2]).max()) for b, r in enumerate(runs))
    print(f"bf16 {tag}: worst rel L2 {worst:.2e}")
    assert worst <= 2e-2, (tag, worst)
    return worst


# ------------------------------------------------------------------------------------------------------------------ fp32
@pytest.mark.parametrize("preset,setting", tc.FP32_MODELS)
def test_fp32_one_row_every_attention_and_finished_row_form(preset, setting):
    """One sequence (the prompt shape of golden tts_stats_greedy: 47 -> 71 cached positions over 8 splits, so the peaks wander through
    the splits and some splits hold no mass worth naming): `fr_one` 1 / 0 (row_gemm_fr1_k's E[q^2] - mean^2 epilogue / split-K slabs
    and the PRO_LN prologue) x `attn_fast` 1 / 0 (one maximum per wave / a rescale per visit)."""
    key = tc.stats_key(setting)
    a, sd, _ = tc.checkpoint(preset, key)
    p, res, want, toks = tc.tts_run(preset, key, -1)
    n, L = len(toks), a.num_decoder_layers
    pl = _plan(a, "fp32", 1)
    assert pl[1] == 0 and pl[2] == 8 and p[0].shape[1] + p[2].shape[1] + n >= 8 * pl[2], pl
    eng = _engine(a, sd, "fp32", 1)
    for fr_one in (1, 0):
        for fast in (1, 0):
            eng.set_option("fr_one", fr_one)
            eng.set_option("attn_fast", fast)
            assert f"|r1={fr_one},{fast}," in eng.options()
            c0 = eng.launch_counts()
            got, gen, lg = eng.inference_tts(p[0].cuda(), p[1].cuda(), p[2].cuda(), **tc.KNOBS, _logit_steps=n)
            c = _delta(eng.launch_counts(), c0)
            assert c["rows_attn"] >= L * (n - 1) and c["tile_attn"] == L, c
            assert (c["row_gemm_fr1"] >= L * (n - 1)) if (fr_one and pl[8] == 1) else (c["row_gemm_fr1"] == 0), (fr_one, pl[8], c)
            assert np.array_equal(got.cpu().numpy(), res), (fr_one, fast)
            d = _worst_abs(lg.cpu().numpy(), want)
            print(f"fp32 one row {preset} {setting} fr_one={fr_one} attn_fast={fast}: worst |d| {d:.2e}")
            assert d <= 1e-3, (fr_one, fast, d)


@pytest.mark.parametrize("B", [3, 8, 12])
@pytest.mark.parametrize("preset,setting", tc.FP32_MODELS)
def test_fp32_finished_rows(preset, setting, B):
    """3 / 8 / 12 ragged sequences on finished rows, consumers on the producers' centred copy (`hq` 1: PRO_LNQ, centred on the mean the
    previous LayerNorm found - the drift of setting A moves it by d_model-independent 4 per update) and on the fp32 rows (`hq` 0:
    PRO_LNW).  3 sequences: 4 attention splits merged in the out-projection; 8: 2 splits; 12: unsplit, normalised in the kernel."""
    key = tc.stats_key(setting)
    a, sd, _ = tc.checkpoint(preset, key)
    runs, _, n = _batch(preset, key, B)
    L = a.num_decoder_layers
    pl = _plan(a, "fp32", B)
    assert pl[1] == 1 and pl[2] == {3: 4, 8: 2, 12: 1}[B], pl
    eng = _engine(a, sd, "fp32", B)
    eng.set_option("shrink", 0)                       # every step at the full width: the form under test all the way
    for hq in (1, 0):
        eng.set_option("hq", hq)
        assert eng.options().split("|fr=")[1].split("|")[0].endswith(f",{hq}")
        c0 = eng.launch_counts()
        outs, lg = _multi(eng, runs, n=n)
        c = _delta(eng.launch_counts(), c0)
        assert c["rows_gemm_fr"] + c["rows_gemm_frp"] >= 2 * L * (n - 1) and c["mt2"] + c["mt4"] + c["wd"] == 0, c
        assert (c["rows_gemm_qp"] >= (L - 1) * (n - 1)) if (hq and pl[9] == 2) else (c["rows_gemm_qp"] == 0), (hq, pl[9], c)
        _check_multi_fp32(runs, outs, lg, f"{preset} {setting} {B} rows hq={hq}")


@pytest.mark.parametrize("preset,setting,B", tc.FP32_WIDE)
def test_fp32_wide_steps_ragged(preset, setting, B):
    """20 / 40 ragged sequences: wide steps (rows_gemm_wd_k, ln_rows_k's centring per row, unsplit attention on a B-row grid)."""
    key = tc.stats_key(setting)
    a, sd, _ = tc.checkpoint(preset, key)
    runs, _, n = _batch(preset, key, B)
    assert len({r[0][2].shape[1] for r in runs}) > 4 and len({len(r[3]) for r in runs}) > 4          # ragged prompts and lengths
    pl = _plan(a, "fp32", B)
    assert pl[1] == 2 and pl[11] == 1, pl
    eng = _engine(a, sd, "fp32", B)
    eng.set_option("shrink", 0)
    c0 = eng.launch_counts()
    outs, lg = _multi(eng, runs, n=n)
    c = _delta(eng.launch_counts(), c0)
    L = a.num_decoder_layers
    assert c["wd"] >= 4 * L * (n - 1) and c["ln_rows"] >= (2 * L + 1) * (n - 1) and c["rows_gemm_fr"] + c["rows_gemm_frp"] == 0, c
    _check_multi_fp32(runs, outs, lg, f"{preset} {setting} {B} rows wide")


@pytest.mark.parametrize("preset,setting", tc.FP32_EDIT)
def test_fp32_two_span_edit(preset, setting):
    """`inference` with two spans (tiny128 / B is golden edit_stats_2span): the one-row steps plus the three-row feed at the span switch."""
    key = tc.stats_key(setting)
    a, sd, _ = tc.checkpoint(preset, key)
    p, mi, res, want, toks = tc.edit_run(preset, key)
    eng = _engine(a, sd, "fp32", 1)
    c0 = eng.launch_counts()
    got, lg = eng.inference(p[0].cuda(), p[1].cuda(), p[2].cuda(), mi, top_k=1, stop_repetition=-1, _logit_steps=len(toks))
    c = _delta(eng.launch_counts(), c0)
    assert c["tile_attn"] == a.num_decoder_layers and c["rows_attn"] >= a.num_decoder_layers * (len(toks) - 1), c
    assert np.array_equal(got.cpu().numpy(), res)
    d = _worst_abs(lg.cpu().numpy(), want)
    print(f"fp32 edit {preset} {setting}: worst |d| {d:.2e}")
    assert d <= 1e-3, d


@pytest.mark.parametrize("preset,setting", tc.FP32_LONG)
def test_fp32_prefill_of_211_rows_through_tile_attn(preset, setting):
    """A 211-row prompt (20 phonemes + 191 columns): thirteen full 16-row tiles and a ragged one of 3 rows through tile_attn_k's online
    softmax, every tile's causal diagonal inside rows whose softmax is peaked; then 14 decode steps over 211 -> 225 cached positions."""
    key = tc.stats_key(setting)
    a, sd, _ = tc.checkpoint(preset, key)
    p, res, want, toks = tc.long_run(preset, key)
    rows = p[0].shape[1] + p[2].shape[1] + 1
    assert rows >= 200 and rows % 16 != 0 and len(toks) <= 40
    eng = _engine(a, sd, "fp32", 1)
    c0 = eng.launch_counts()
    got, gen, lg = eng.inference_tts(p[0].cuda(), p[1].cuda(), p[2].cuda(), **tc.KNOBS, _logit_steps=len(toks))
    c = _delta(eng.launch_counts(), c0)
    L = a.num_decoder_layers
    assert c["tile_attn"] == L and c["tile_attn64"] == 0 and c["ln_rows"] >= 2 * L, c
    assert np.array_equal(got.cpu().numpy(), res)
    d = _worst_abs(lg.cpu().numpy(), want)
    print(f"fp32 prefill {preset} {setting}: worst |d| {d:.2e}")
    assert d <= 1e-3, d


# ------------------------------------------------------------------------------------------------------------------ bf16
BF16_MODELS = [("tiny128", "A"), ("tiny128", "B"), ("tiny_h16", "A"), ("tiny_h16", "B")]      # d = 512: the centred copy and rows_gemm_qp_k are taken


@pytest.mark.parametrize("preset,setting", BF16_MODELS)
def test_bf16_one_row(preset, setting):
    key = tc.stats_key(setting, bf16=True)
    a, sd, _ = tc.checkpoint(preset, key)
    p, res, want, toks = tc.tts_run(preset, key, -1)
    n, L = len(toks), a.num_decoder_layers
    eng = _engine(a, sd, "bf16", 1)
    for fr_one, fast in ((1, 1), (0, 1), (1, 0)):
        eng.set_option("fr_one", fr_one)
        eng.set_option("attn_fast", fast)
        assert f"|r1={fr_one},{fast}," in eng.options()
        c0 = eng.launch_counts()
        got, gen, lg = eng.inference_tts(p[0].cuda(), p[1].cuda(), p[2].cuda(), **tc.KNOBS, _forced=toks, _logit_steps=n)
        c = _delta(eng.launch_counts(), c0)
        assert ((c["row_gemm_fr1"] >= L * (n - 1)) if fr_one else (c["row_gemm_fr1"] == 0)) and c["rows_attn"] >= L * (n - 1), c
        rel = float(rel_l2(lg.cpu().numpy(), want).max())
        print(f"bf16 one row {preset} {setting} fr_one={fr_one} attn_fast={fast}: worst rel L2 {rel:.2e}")
        assert rel <= 2e-2, (fr_one, fast, rel)


BF16_FR_MODES = {"default": {}, "hq0": {"hq": 0}, "p32": {"att_p16": 0}, "qkv12": {"qkv_p8": 1}}


@pytest.mark.parametrize("B", [2, 4, 8])
@pytest.mark.parametrize("preset,setting", BF16_MODELS)
def test_bf16_finished_rows(preset, setting, B):
    """2 / 4 / 8 rows: the centred bf16 copy behind rows_gemm_qp_k (var = E[q^2] - mean(q)^2 on rows centred on the PREVIOUS mean), bf16 /
    fp32 attention partials in the out-projection's split merge, the QKV projection on 8- / 12-channel tiles."""
    key = tc.stats_key(setting, bf16=True)
    a, sd, _ = tc.checkpoint(preset, key)
    runs, forced, n = _batch(preset, key, B)
    L = a.num_decoder_layers
    pl = _plan(a, "bf16", B)
    assert pl[1] == 1 and pl[2] >= 2 and pl[9] == 2, pl
    eng = _engine(a, sd, "bf16", B)
    eng.set_option("shrink", 0)
    for mode, opts in BF16_FR_MODES.items():
        for name, v in {"hq": 1, "att_p16": 1, "qkv_p8": 2, **opts}.items():
            eng.set_option(name, v)
        c0 = eng.launch_counts()
        outs, lg = _multi(eng, runs, forced, n)
        c = _delta(eng.launch_counts(), c0)
        assert c["rows_gemm_fr"] + c["rows_gemm_frp"] >= 2 * L * (n - 1), c
        assert (c["rows_gemm_qp"] >= (L - 1) * (n - 1)) if mode in ("default", "p32") else (c["rows_gemm_qp"] == 0), (mode, c)
        _check_multi_bf16(runs, lg, f"{preset} {setting} {B} rows {mode}")


@pytest.mark.parametrize("preset,setting", BF16_MODELS)
def test_bf16_twelve_rows(preset, setting):
    key = tc.stats_key(setting, bf16=True)
    a, sd, _ = tc.checkpoint(preset, key)
    runs, forced, n = _batch(preset, key, 12)
    pl = _plan(a, "bf16", 12)
    assert pl[1] == 1 and pl[2] == 1, pl                # finished rows, unsplit attention that normalises itself
    eng = _engine(a, sd, "bf16", 12)
    eng.set_option("shrink", 0)
    c0 = eng.launch_counts()
    outs, lg = _multi(eng, runs, forced, n)
    c = _delta(eng.launch_counts(), c0)
    assert c["rows_gemm_fr"] + c["rows_gemm_frp"] >= 2 * a.num_decoder_layers * (n - 1) and c["rows_gemm_qp"] == 0, c
    _check_multi_bf16(runs, lg, f"{preset} {setting} 12 rows")


@pytest.mark.parametrize("preset,setting,B", [("tiny128", "A", 20), ("tiny_h16", "B", 20), ("tiny_h16", "A", 40), ("tiny128", "B", 40)])
def test_bf16_wide_steps(preset, setting, B):
    """20 / 40 rows: the linear layers on rows_gemm_wd_k / the weight-stationary rows_gemm_mt_k, the heads once over all rows / 16 rows
    at a time; ln_rows_k centres every row before it rounds."""
    key = tc.stats_key(setting, bf16=True)
    a, sd, _ = tc.checkpoint(preset, key)
    runs, forced, n = _batch(preset, key, B)
    assert _plan(a, "bf16", B)[1] == 2
    eng = _engine(a, sd, "bf16", B)
    eng.set_option("shrink", 0)
    for wg in (1, 0):
        for wh in (1, 0):
            eng.set_option("wide_gemm", wg)
            eng.set_option("wide_heads", wh)
            c0 = eng.launch_counts()
            outs, lg = _multi(eng, runs, forced, n)
            c = _delta(eng.launch_counts(), c0)
            assert (c["wd"] > 0 and c["mt2"] + c["mt4"] == 0) if wg else (c["mt2"] + c["mt4"] > 0 and c["wd"] == 0), (wg, wh, c)
            assert wh or c["rows_gemm"] > 0, (wg, wh, c)              # the heads 16 rows at a time on the rows-GEMM
            assert c["ln_rows"] >= (2 * a.num_decoder_layers + 1) * (n - 1), c
            _check_multi_bf16(runs, lg, f"{preset} {setting} {B} rows wide_gemm={wg} wide_heads={wh}")


@pytest.mark.parametrize("setting", ["A", "B"])
def test_bf16_prefill_of_211_rows_on_both_tile_kernels(setting):
    """tiny128 (head_dim 128): the 211-row prompt through tile_attn_k (16-row tiles) and tile_attn64_k (64-row blocks, "2,128")."""
    key = tc.stats_key(setting, bf16=True)
    a, sd, _ = tc.checkpoint("tiny128", key)
    p, res, want, toks = tc.long_run("tiny128", key)
    eng = _engine(a, sd, "bf16", 1)
    L = a.num_decoder_layers
    for opt, k64 in (("1", 0), ("2,128", L)):
        eng.set_option("tile_attn", opt)
        c0 = eng.launch_counts()
        got, gen, lg = eng.inference_tts(p[0].cuda(), p[1].cuda(), p[2].cuda(), **tc.KNOBS, _forced=toks, _logit_steps=len(toks))
        c = _delta(eng.launch_counts(), c0)
        assert c["tile_attn"] == L and c["tile_attn64"] == k64, (opt, c)
        rel = float(rel_l2(lg.cpu().numpy(), want).max())
        print(f"bf16 prefill tiny128 {setting} tile_attn={opt}: worst rel L2 {rel:.2e}")
        assert rel <= 2e-2, (opt, rel)


def test_bf16_eval_forward_on_setting_a():
    """One vc_eval_forward call (block GEMMs + ce_rows_k) on setting A against the oracle's objective, on the bars of
    tests/test_gpu_forward.py: the same number of targets, loss within 2e-2 relative, top-10 hits within 3 % of the targets."""
    from oracle.gen_golden import forward_inputs
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from voicecraft_amd import synth
    # the terminator is a target here: not muted (its -1e4 bias would be most of the loss), and twelve of the sixteen token ids the
    # batch uses are boosted so that the top-10 metric has hits and misses (oracle/gen_golden.py FORWARD_CASES)
    a = synth.make_args("tiny128", num_decoder_layers=tc.LAYERS["tiny128"])
    sd = synth.trained_stats(synth.make_state_dict(a, seed=tc.WSEED, mute_eos=False, boost=[(-1, t, 4.0) for t in range(12)]), a,
                             **tc.stats_kw("A", k_bias=8.0))
    orc = VoiceCraftOracle(a, sd)
    spec = dict(samples=[(10, 70, 27), (6, 52, 28)])
    spans = [[(1, 6), (30, 44)], [(26, 51)]]
    batch = forward_inputs(spec, a)
    want = orc.forward(batch, spans)
    eng = _engine(a, sd, "bf16", 2, max_positions=512)
    c0 = eng.launch_counts()
    out = eng.forward({k: v.cuda() for k, v in batch.items()}, spans)
    c = _delta(eng.launch_counts(), c0)
    assert c["blk64"] + c["blk64_occ2"] + c["blk128_sbs"] + c["blk128_2x2"] > 0 and c["tile_attn"] > 0, c
    assert int(out["effective_ntoken"]) == int(want["effective_ntoken"])
    rel = abs(float(out["loss"]) - float(want["loss"])) / abs(float(want["loss"]))
    print(f"bf16 eval_forward A: worst loss {float(out['loss']):.3f} against {float(want['loss']):.3f} (rel {rel:.2e}), "
          f"hits {float(out['top10acc']):.0f} against {float(want['top10acc']):.0f} of {int(want['effective_ntoken']) // a.n_codebooks}")
    assert rel <= 2e-2, rel
    assert abs(float(out["top10acc"]) - float(want["top10acc"])) <= 0.03 * float(want["effective_ntoken"]) / a.n_codebooks


# ------------------------------------------------------------------------------------------------------------------ the drift sweep
@pytest.mark.parametrize("preset", ["tiny128", "tiny_h16"])
def test_bf16_centred_copy_holds_the_bar_at_every_drift(preset):
    """bf16, 4 rows, setting A with a common bias component (`drift`) of 0 / 4 / 32 per residual update.  The consumers read rows the
    PRODUCER rounded to bf16 after centring them (`hq` 1); a copy centred on the mean the row had BEFORE the producer's own update would
    be off by the update's mean, `drift`, and at 32 spend the mantissa on it (emulated: 2.4e-2).  The producer therefore centres on
    the previous mean PLUS the mean of the bias it adds; both forms must hold the bar at every drift."""
    worst = {}
    for drift in (0.0, 4.0, 32.0):
        key = tc.stats_key("A", bf16=True, drift=drift)
        a, sd, _ = tc.checkpoint(preset, key)
        runs, forced, n = _batch(preset, key, 4)
        eng = _engine(a, sd, "bf16", 4)
        eng.set_option("shrink", 0)
        for hq in (0, 1):
            eng.set_option("hq", hq)
            c0 = eng.launch_counts()
            outs, lg = _multi(eng, runs, forced, n)
            c = _delta(eng.launch_counts(), c0)
            assert (c["rows_gemm_qp"] >= (a.num_decoder_layers - 1) * (n - 1)) if hq else (c["rows_gemm_qp"] == 0), (hq, c)
            lg = lg.cpu().numpy()
            worst[(drift, hq)] = max(float(rel_l2(lg[: len(r[2]), b], r[2]).max()) for b, r in enumerate(runs))
        del eng
    print(f"drift sweep {preset}:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) <= 2e-2, worst
