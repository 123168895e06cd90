"""-m gpu: the token side of the model away from K = 4 codebooks / V = 2052 / head_hidden 1024.

vc_create accepts 2..8 codebooks, any V = audio_vocab_size + n_special up to 2176 and any head_hidden that is a multiple
of 256; every other GPU test runs one point of that range.  Here the reference-made fixtures of oracle/gen_golden.py for
K = 2, 3, 5, 6, 8, audio vocabularies 512 / 1024 / 1536 (head_hidden 256 / 512 / 768) and V = 2176 go through the engine:

  one sequence     fp32 result equal to the reference's (greedy free-running, sampled by replaying the recorded draws), with
                   and without graph replay; fp32 head logits of every step within 1e-3 of the oracle; bf16 teacher-forced
                   logits within 2e-2 relative L2 (rel_l2 of test_gpu_model.py) and the assembled result identical
  several rows     3 / 12 / 20 sequences per step, fp32 greedy free-running, each equal to its own oracle run, the launch
                   census telling which form ran (head_hidden 768 has no wide-decode form: the fallback kernel)
  editing batch    inference_multi at K = 8 with 1 / 2 / 2 spans: the one-row feed steps of a span switch
  streaming        frames handed out never run ahead of `finished steps - (K - 1)`
  objective        vc_eval_forward on fwd_k8 / fwd_k2_av1024, K per-codebook sums
  sampler          vc_debug_sample at the vocabulary edges (V = 1 .. 2176), top_k above 64 / at V / past V, degenerate rows

The bars are the project's own (test_gpu_model.py, test_gpu_forward.py, test_gpu_sampler.py); each test prints its
figures before it asserts."""
import functools
import os

import numpy as np
import pytest
import torch
from scipy import stats

from _util import GOLDEN, MODEL_CASES, build_case, build_forward_case, load_golden, run_oracle_case
from test_gpu_model import engine_run, make_engine, rel_l2
from test_gpu_sampler import N_DRAWS, chi_square, expected_probs, top_p_boundary_is_clear

pytestmark = pytest.mark.gpu

# K <= 6 and the small vocabularies first, K = 8 last
NEW_CASES = ["tts_k2_greedy", "tts_k3_sampled_eos", "edit_k2_sampled_eog", "tts_k5_av1024_hd128", "tts_av512_oldscheme",
             "tts_batch3_k6_av1536", "tts_vcap", "tts_k8_greedy", "tts_k8_sampled_eos", "edit_k8_2span"]
NEW_SAMPLED = [n for n in NEW_CASES if "tseed" in MODEL_CASES[n]]


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """(res, trace) of the oracle on a golden case (seeded as the reference was: its trajectory is the fixture's).  Computed
    once per case and shared; nobody writes to it."""
    torch.set_num_threads(min(4, torch.get_num_threads()))
    trace = []
    res, _ = run_oracle_case(name, trace=trace)
    return res.numpy(), trace


def test_the_new_cases_cover_the_shapes_they_are_named_for():
    shapes = set()
    for name in NEW_CASES:
        _, a, _, _, _, _ = build_case(name)
        shapes.add((a.n_codebooks, a.audio_vocab_size + a.n_special, a.audio_vocab_size // 2))
    assert {s[0] for s in shapes} == {2, 3, 4, 5, 6, 8}
    assert {s[1] for s in shapes} == {515, 1028, 1540, 2052, 2176}
    assert {s[2] for s in shapes} == {256, 512, 768, 1024}
    for name in NEW_SAMPLED + ["edit_k8_2span"]:                      # the un-muted terminator really ends these before the cap
        g = load_golden(name)
        if "gen" in g.files:
            assert 0 < g["gen"].shape[2] < 10 * g["x"].shape[1] - g["y"].shape[1], name
    g = load_golden("tts_k8_sampled_eos")                             # ... and K = 8 has its 8-step staggered tail
    assert int(g["n_steps"]) == g["gen"].shape[2] + 8


# ------------------------------------------------------------------------------------------------ one sequence
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("name", NEW_CASES)
def test_fp32_result_equals_the_reference(name, graph):
    """Greedy cases free-running; sampled cases with the fixture's recorded raw draws replayed through the device state
    machine (forced_mode = draws) - the K-1 `empty` overrides, the K-step staggered EOG tail, the span switch, the keep-LAST
    rule of the best-of-3 case - to exactly the reference's result."""
    g = load_golden(name)
    eng, spec, x, x_lens, y = make_engine(name, "fp32", use_graph=graph)
    if name in NEW_SAMPLED:
        res, _ = engine_run(eng, spec, x, x_lens, y, forced=g["draws"], forced_mode="draws", seed=99)
    else:
        res, _ = engine_run(eng, spec, x, x_lens, y)
    assert list(res.shape) == list(g["res"].shape), (res.shape, g["res"].shape)
    assert np.array_equal(res.cpu().numpy(), g["res"]), "token ids differ from the reference"


def _teacher_forced(name, dtype, graph):
    """-> (res, want_res, got [n, R, K, V], want [n, R, K, V], live [n, R]): the engine's raw head logits of every step of the
    oracle's trajectory.  One sequence: the step's final tokens are forced.  Best-of-N: the recorded draws are replayed (the
    trace holds the final tokens of the kept sample only); every sample is compared until the group is decided, the kept one
    alone afterwards (the engine drops the others, their logits rows stay zero)."""
    want_res, trace = oracle_run(name)
    n = len(trace)
    eng, spec, x, x_lens, y = make_engine(name, dtype, use_graph=graph)
    if spec["mode"] != "tts_batch":
        want = torch.stack([t["logits"][0] for t in trace]).numpy()[:, None]
        forced = torch.stack([t["tokens"] for t in trace]).numpy()
        res, lg = engine_run(eng, spec, x, x_lens, y, forced=forced, logit_steps=n)
        return res.cpu().numpy(), want_res, lg.cpu().numpy()[:, None], want, np.ones((n, 1), dtype=bool)
    g = load_golden(name)
    out = eng.inference_tts_batch(x, x_lens, y, **spec["knobs"], _forced=g["draws"], _forced_mode="draws", _seed=5, _logit_steps=n)
    got = out[2].cpu().numpy()                                                   # [n, N, K, V]
    want = torch.stack([t["logits"] for t in trace]).numpy()
    term = int(eng.args.eos)
    decided = min(s for s, t in enumerate(trace) if int(t["tokens"][0]) == term)
    kept = [b for b in range(got.shape[1]) if np.any(got[-1, b] != 0)]
    assert len(kept) == 1 and decided < n - 1, (kept, decided, n)
    live = np.zeros(got.shape[:2], dtype=bool)
    live[: decided + 1] = True
    live[:, kept[0]] = True
    assert not np.any(got[decided + 1:][~live[decided + 1:]] != 0)              # dropped samples write nothing more
    return out[0].cpu().numpy(), want_res, got, want, live


@pytest.mark.parametrize("name", NEW_CASES)
def test_fp32_logits_of_every_step_close_to_oracle(name):
    res, want_res, got, want, live = _teacher_forced(name, "fp32", False)
    assert np.array_equal(res, want_res)
    err = np.abs(got - want).max(axis=(2, 3))
    worst = float(err[live].max())
    print(f"{name}: fp32 logits max|d| over {len(got)} steps = {worst:.3e}")
    assert worst <= 1e-3, f"fp32 logits max|d| per step: {np.where(live, err, 0).max(axis=1)}"


@pytest.mark.parametrize("name", NEW_CASES)
def test_bf16_teacher_forced_logits(name):
    res, want_res, got, want, live = _teacher_forced(name, "bf16", True)
    worst = 0.0
    for b in range(got.shape[1]):
        steps = np.flatnonzero(live[:, b])
        worst = max(worst, float(rel_l2(got[steps, b], want[steps, b]).max()))
    print(f"{name}: bf16 relative L2 worst step = {worst:.4f}")
    # teacher forcing replays the reference trajectory, so the assembled output must be identical
    assert np.array_equal(res, want_res)
    assert worst <= 2e-2, f"bf16 relative L2 error per step: max {worst:.4f}"


# ------------------------------------------------------------------------------------------------ several rows per step
MULTI = {
    "k8": ("tiny", dict(n_codebooks=8), 31),
    "k2": ("tiny", dict(n_codebooks=2), 32),
    "k5_av1024": ("tiny128", dict(n_codebooks=5, audio_vocab_size=1024), 33),       # V = 1028, head_hidden 512
    "k6_av1536": ("tiny", dict(n_codebooks=6, audio_vocab_size=1536), 34),          # V = 1540, head_hidden 768: no wide form
}


@functools.lru_cache(maxsize=None)
def _multi_model(key):
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from voicecraft_amd import synth
    preset, kw, seed = MULTI[key]
    a = synth.make_args(preset, **kw)
    sd = synth.make_state_dict(a, seed=seed)
    return a, sd, VoiceCraftOracle(a, sd)


@functools.lru_cache(maxsize=None)
def _multi_want(key, u):
    """Prompt u of a model and its own oracle run (greedy).  Ragged: 2..4 phonemes and 5..13 prompt frames give 7..35
    generated frames (the terminator is muted: the reference's 10-frames-per-phoneme cap ends a sequence), so the sequences
    of a batch retire on different steps."""
    from voicecraft_amd import synth
    a, sd, orc = _multi_model(key)
    torch.set_num_threads(min(4, torch.get_num_threads()))
    x, xl, y = synth.random_prompt(a, 2 + u % 3, 5 + 2 * (u % 5), seed=900 + u)
    return x, y, orc.inference_tts(x, xl, y, top_k=1, stop_repetition=3)[0].numpy()


@pytest.mark.parametrize("key,B", [("k2", 3), ("k2", 12), ("k2", 20), ("k5_av1024", 3), ("k5_av1024", 12), ("k5_av1024", 20),
                                   ("k6_av1536", 20), ("k8", 3), ("k8", 12), ("k8", 20)])
def test_fp32_multi_utterance_tokens_equal_per_sequence_oracle(key, B):
    """3 sequences: the finished-row form of 2..8 rows; 12: its 9..16-row form (unsplit attention, two rows per consumer
    wave); 20: the wide-decode form of 17..64 rows, the heads as one grouped GEMM over K groups - on rows_gemm_wd_k where
    head_hidden has a k-tile count per wave (256 / 512 / 1024), on the weight-stationary fallback where it has none (768).
    As the batch shrinks it is re-packed onto the narrower forms.  The census counts what is launched outside a graph
    replay, i.e. the capture of every width the call passes through."""
    from voicecraft_amd.engine import VoiceCraftEngine
    a, sd, _ = _multi_model(key)
    want = [_multi_want(key, u) for u in range(B)]
    assert len({w[2].shape[2] for w in want}) >= 3                               # ragged results
    eng = VoiceCraftEngine(a, sd, device="cuda:0", dtype="fp32", max_seqs=B, max_positions=512)
    c0 = eng.launch_counts()
    outs = eng.inference_tts_multi([w[0][0] for w in want], [w[1][0] for w in want], top_k=1, stop_repetition=3)
    c = _delta(eng.launch_counts(), c0)
    repacks = int(eng.debug_read("host_ms", (8,), torch.float64)[6])
    print(f"{key} B={B}: census {dict((k, v) for k, v in c.items() if v)}, re-packs {repacks}")
    for u, ((x, y, w), (res, gen)) in enumerate(zip(want, outs)):
        got = res.cpu().numpy()
        assert got.shape == w.shape and np.array_equal(got, w), (key, B, u)
    assert c["rows_gemm_fr"] + c["rows_gemm_frp"] > 0, c                         # every size gets to 2..16 rows, at the latest as it shrinks
    if B <= 16:
        assert c["wd"] == 0 and c["mt2"] + c["mt4"] == 0, c
    elif a.audio_vocab_size // 2 == 768:
        assert c["wd"] == 0 and c["mt2"] + c["mt4"] > 0, c                       # the fallback kernel
    else:
        assert c["wd"] > 0 and c["mt2"] + c["mt4"] == 0, c
    if B >= 12:
        assert repacks >= 1, repacks


def test_fp32_batched_editing_at_eight_codebooks():
    """inference_multi, 3 requests with 1, 2 and 2 spans at K = 8: a span switch is fed over three one-row steps here (the
    single call's 3-row step is covered by edit_k8_2span above).  Request 1 is the reference-made fixture; every request
    equals its own `inference` call and the oracle."""
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from voicecraft_amd import synth
    from voicecraft_amd.engine import VoiceCraftEngine
    spec, args, sd, x1, _, y1 = build_case("edit_k8_2span")
    kn = dict(spec["knobs"])
    kn.pop("kvcache")
    xa, _, ya = synth.random_prompt(args, 11, 40, seed=951)
    xc, _, yc = synth.random_prompt(args, 12, 52, seed=952)
    reqs = [(xa, ya, [(12, 19)]), (x1, y1, spec["spans"]), (xc, yc, [(5, 9), (30, 38)])]
    eng = VoiceCraftEngine(args, sd, device="cuda:0", dtype="fp32", max_seqs=4, max_positions=512)
    outs = eng.inference_multi([r[0][0] for r in reqs], [r[1][0] for r in reqs], [r[2] for r in reqs], **kn)
    assert np.array_equal(outs[1].cpu().numpy(), load_golden("edit_k8_2span")["res"])
    torch.set_num_threads(min(4, torch.get_num_threads()))
    orc = VoiceCraftOracle(args, sd)
    for b, ((x, y, spans), got) in enumerate(zip(reqs, outs)):
        got = got.cpu().numpy()
        mi = torch.tensor([spans], dtype=torch.int64)
        xl = torch.tensor([x.shape[1]])
        want = orc.inference(x, xl, y, mi, **kn).numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (b, spans)
        one = eng.inference(x.cuda(), xl.cuda(), y.cuda(), mi, **kn).cpu().numpy()
        assert np.array_equal(got, one), (b, spans)


# ------------------------------------------------------------------------------------------------ streaming
@pytest.mark.parametrize("graph_steps", [1, 8])
@pytest.mark.parametrize("name", ["tts_k2_greedy", "tts_k8_greedy"])
def test_stream_never_runs_ahead_of_the_delay_pattern(name, graph_steps):
    """Frame t is complete once step t + K - 1 has ended (out[j][t] = rows[j + t][j]).  After every `next` of a live
    sequence the frames handed out so far must not exceed `finished steps - (K - 1)`; the chunks are the blocking call's
    frames, which are the reference's."""
    g = load_golden(name)
    eng, spec, x, x_lens, y = make_engine(name, "fp32")
    eng.set_option("graph_steps", graph_steps)
    K = eng.args.n_codebooks
    kw = dict(spec["knobs"], _seed=1)
    res, gen = eng.inference_tts(x, x_lens, y, **kw)
    assert np.array_equal(res.cpu().numpy(), g["res"])
    chunks, at, live_checks = [], 0, 0
    for first, codes in eng.inference_tts_stream(x, x_lens, y, chunk_frames=1, **kw):
        assert first == at and codes.shape[:2] == (1, K)
        chunks.append(codes.clone())
        at += codes.shape[2]
        rows, emitted, over = (int(v) for v in eng.debug_read("stream", (3,), torch.int32))
        assert emitted == at
        if not over:
            assert emitted <= rows - (K - 1), (emitted, rows, K)
            live_checks += emitted > 0
    assert live_checks >= 2, live_checks                       # frames really arrived while the sequence was live
    assert torch.equal(torch.cat(chunks, dim=2), gen)
    assert torch.equal(eng.last_stream_result[0], res)


# ------------------------------------------------------------------------------------------------ training objective
@pytest.mark.parametrize("name", ["fwd_k2_av1024", "fwd_k8"])
def test_forward_objective_with_other_codebook_counts(name):
    """vc_eval_forward against the reference-made fixture (tolerances of test_gpu_forward.py: fp32 loss 2e-4 relative, hits
    and target count exact; bf16 loss 2e-2, hits within 3 %), and the K per-codebook sums against the oracle's."""
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from test_gpu_forward import engine_for
    spec, args, sd, batch = build_forward_case(name)
    g = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    K = args.n_codebooks
    cu = {k: v.cuda() for k, v in batch.items()}
    out = engine_for(args, sd, "fp32").forward(cu, spec["spans"], _per_row=True)
    print(f"{name}: fp32 loss {float(out['loss']):.4f} (reference {float(g['loss']):.4f})")
    assert int(out["effective_ntoken"]) == int(g["effective_ntoken"])
    assert abs(float(out["loss"]) - float(g["loss"])) <= 2e-4 * abs(float(g["loss"])), (float(out["loss"]), float(g["loss"]))
    hits = np.array([float(t) for t in out["top10acc_by_codebook"]])
    assert len(hits) == K == len(g["top10acc_by_codebook"]) and len(out["_nll_sum"]) == K
    assert np.array_equal(np.rint(hits), np.rint(g["top10acc_by_codebook"])), (hits, g["top10acc_by_codebook"])
    ref = VoiceCraftOracle(args, sd).forward(batch, spec["spans"])
    lg, tg = ref["_per_token_logits"], ref["_targets"]                            # [K,N,V], [K,N]
    for k in range(K):
        want = float(torch.nn.functional.cross_entropy(lg[k].double(), tg[k], reduction="sum"))
        assert abs(out["_nll_sum"][k] - want) <= 2e-4 * abs(want), (k, out["_nll_sum"][k], want)
    assert out["_nll_rows"].shape[1] == K and out["_tgt_rows"].shape[1] == K
    b16 = engine_for(args, sd, "bf16").forward(cu, spec["spans"])
    print(f"{name}: bf16 loss {float(b16['loss']):.4f}, hits {float(b16['top10acc']):.0f} (reference {float(g['top10acc']):.0f})")
    assert int(b16["effective_ntoken"]) == int(g["effective_ntoken"])
    assert abs(float(b16["loss"]) - float(g["loss"])) <= 2e-2 * abs(float(g["loss"]))
    assert abs(float(b16["top10acc"]) - float(g["top10acc"])) <= 0.03 * float(g["effective_ntoken"]) / K


# ------------------------------------------------------------------------------------------------ device sampler
def _row(V, seed, scale):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(V) * scale).astype(np.float32))


def _clear_row(V, top_k, top_p, temperature, scale, seed=21, edit=None, min_big=0):
    """A random row whose nucleus boundary is unambiguous (top_p_boundary_is_clear), after `edit(row)`; min_big: with at
    least that many tokens expected 8 times or more (a row of large scale is not ONE token and nothing else)."""
    while True:
        row = _row(V, seed, scale)
        if edit is not None:
            edit(row)
        if top_p_boundary_is_clear(row, top_k, top_p, temperature) and \
                (not min_big or (expected_probs(row, top_k, top_p, temperature)[0] * N_DRAWS >= 8).sum() >= min_big):
            return row
        seed += 1


def check_distribution(row, top_k, top_p, temperature, seed):
    """The acceptance of test_gpu_sampler.py: nothing outside the oracle's support (no padding column either), every token
    expected 30 times or more is seen, Pearson chi-square below the 1 - 1e-6 quantile with bins of expectation < 8 pooled."""
    from voicecraft_amd.engine import debug_sample
    V = row.numel()
    probs, filt = expected_probs(row, top_k, top_p, temperature)
    toks = debug_sample(row.cuda(), N_DRAWS, top_k=top_k, top_p=top_p, temperature=temperature, seed=seed).cpu().numpy()
    assert toks.min() >= 0 and toks.max() < V, (toks.min(), toks.max(), V)       # never a padding column
    counts = np.bincount(toks, minlength=V)
    support = np.isfinite(filt.numpy())
    assert counts[~support].sum() == 0, f"{counts[~support].sum()} draws outside the oracle's support"
    assert (counts[probs * N_DRAWS >= 30] > 0).all()
    if support.sum() == 1:
        assert counts[support][0] == N_DRAWS
        return counts, support
    stat, dof = chi_square(counts, probs, N_DRAWS)
    if dof >= 1:
        limit = stats.chi2.ppf(1 - 1e-6, dof)
        assert stat < limit, f"chi-square {stat:.1f} over {dof} dof exceeds {limit:.1f}"
    return counts, support


@pytest.mark.parametrize("top_k,top_p", [(40, 1.0), (0, 0.8)])
@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 515, 1028, 2175, 2176])
def test_sampler_vocabulary_edges(V, top_k, top_p):
    """V < 64: lanes that hold no element; V a multiple of 64: no padding lane; 2176: every register slot live; V below top_k:
    the clamp kk = min(top_k, V)."""
    row = _clear_row(V, top_k, top_p, 1.0, 1.5)
    counts, support = check_distribution(row, top_k, top_p, 1.0, 500 + V)
    if top_p >= 1.0:
        assert support.sum() == min(top_k, V)                                    # (no ties in these rows)


@pytest.mark.parametrize("V,top_k", [(2052, 65), (2052, 100), (2052, 500), (2052, 2052), (2052, 2057), (65, 65), (65, 70), (30, 40)])
def test_sampler_threshold_search_past_the_fast_path(V, top_k):
    """top_k > 64 calls the full bitwise search directly; top_k >= V keeps the whole row (padding keys sit below every finite
    key and must stay out)."""
    row = _row(V, 40 + top_k, 1.0)
    counts, support = check_distribution(row, top_k, 1.0, 1.0, 700 + top_k)
    assert support.sum() == min(top_k, V)


def test_sampler_row_of_equal_logits():
    """Every token ties at the threshold: the support is the whole row and the draw is uniform, whatever top_k says."""
    for V in (2052, 2176, 64):
        row = torch.full((V,), 0.75, dtype=torch.float32)
        for top_k in (40, 100):
            counts, support = check_distribution(row, top_k, 1.0, 1.0, 800 + V + top_k)
            assert support.all()


@pytest.mark.parametrize("top_k,top_p", [(40, 1.0), (0, 0.8), (-100, 1.0)])
def test_sampler_row_with_muted_specials(top_k, top_p):
    """Four entries at -1e4, as the synthetic checkpoints mute the special tokens: their probability underflows to zero on the
    device (and in the fp64 expectation), so they are never drawn - filtered or not - and nothing turns into NaN (a NaN row
    would end on the fall-back token of the inverse-CDF walk and fail the distribution)."""
    V = 2052
    def mute(r):
        r[2048:] = -1e4
    row = _clear_row(V, top_k, top_p, 1.0, 1.5, seed=61, edit=mute)
    counts, support = check_distribution(row, top_k, top_p, 1.0, 900 + top_k)
    assert counts[2048:].sum() == 0


@pytest.mark.parametrize("top_k,top_p", [(-100, 1.0), (40, 1.0), (0, 0.8)])
def test_sampler_row_of_large_scale(top_k, top_p):
    """Logits of scale 30: the device's exponentials underflow to zero in the tail, the oracle's expectations there are tiny
    and fall into the pooled bin."""
    row = _clear_row(2052, top_k, top_p, 1.0, 30.0, seed=71, min_big=3)
    if top_k <= 0 and top_p >= 1.0:
        assert (float(row.max()) - row.numpy() > 104.0).sum() > 500              # exp(-104) < the smallest fp32 denormal: these underflow
    check_distribution(row, top_k, top_p, 1.0, 1000 + top_k)
