"""-m gpu: best-of-N sampling inside multi-utterance TTS calls (vc_tts_multi_best_of / inference_tts_multi(batch_size=N) /
inference_tts_long(batch_size=N)).

B utterances x N samples run as B*N sequences; sample j of utterance u sits in slot u*N + j.  Every utterance must give
exactly what inference_tts_batch(batch_size=N) gives on its own prompt - the LAST sample whose first codebook terminates
first is kept (models/voicecraft.py:1296-1302) - also after the batch has been re-packed onto narrower steps, next to
filler rows, and on the wide (17..64-row) step forms.  Draws are replayed (forced_mode = draws) and checked against the
oracle replaying the same draws.
"""
import time

import numpy as np
import pytest
import torch

from _util import build_case, load_golden
from test_gpu_model import rel_l2

pytestmark = pytest.mark.gpu

TERM = 2051                  # eos of the synthetic checkpoints (synth.make_args): the TTS terminator


def engine_for(args, sd, dtype="fp32", **kw):
    from voicecraft_amd.engine import VoiceCraftEngine
    kw.setdefault("max_positions", 256)
    return VoiceCraftEngine(args, sd, device="cuda:0", dtype=dtype, **kw)


def knobs_of(spec):
    kn = dict(spec["knobs"])
    kn.pop("kvcache", None)
    kn.pop("batch_size", None)
    return kn


def design_draws(rs, n, N, K, terms):
    """Random raw draws [n][N][K] (never a special token); terms = {sample: step} puts the terminator on codebook 0."""
    d = rs.randint(0, 2048, size=(n, N, K)).astype(np.int64)
    for j, t in terms.items():
        d[t, j, 0] = TERM
    return d


def run_multi(eng, prompts, N, draws, kn, **kw):
    """prompts: list of (x [1,Lx], x_lens, y [1,T,K]); draws: list of [n][N][K] per utterance -> res arrays."""
    forced = np.concatenate(draws, axis=1) if draws is not None else None
    outs = eng.inference_tts_multi([p[0][0] for p in prompts], [p[2][0] for p in prompts], **kn, batch_size=N, _forced=forced,
                                   _forced_mode="draws", _seed=7, **kw)
    return [o[0].cpu().numpy() for o in outs]


def oracle_best_of(orc, prompt, N, draws, kn, trace=None):
    x, xl, y = prompt
    return orc.inference_tts_batch(x, xl, y, batch_size=N, forced_draws=draws, trace=trace, **kn)[0].numpy()


def repacks(eng):
    return int(eng.debug_read("host_ms", (8,), torch.float64)[6])


def check_kept(res, prompt, draws, kept, t):
    """The kept sample's codebook-0 trajectory: its own draws up to the terminator step t, then the terminator."""
    T = prompt[2].shape[1]
    assert res.shape[2] == T + t, (res.shape, T, t)
    assert np.array_equal(res[0, 0, T:], draws[:t, kept, 0])


@pytest.mark.parametrize("graph", [False, True])
def test_reference_run_inside_a_batch_of_three(graph):
    """The reference's recorded best-of-4 run (tts_batch4_sampled) replayed as utterance 1 of a 3-utterance call (12 rows) must
    give the golden result; utterance 0 (samples 1 and 3 terminate on the same step: 3 is kept) and utterance 2 (only sample 0
    terminates) must equal the oracle replaying their draws.  The three terminators fall on different steps."""
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from voicecraft_amd import synth
    g = load_golden("tts_batch4_sampled")
    spec, args, sd, x1, xl1, y1 = build_case("tts_batch4_sampled")
    kn = knobs_of(spec)
    K, N = args.n_codebooks, 4
    t1 = g["res"].shape[2] - y1.shape[1]
    t0 = 13 if t1 != 13 else 14
    t2 = 17 if t1 != 17 else 18
    n = max(len(g["draws"]), t0 + K + 2, t2 + K + 2)
    rs = np.random.RandomState(11)
    d1 = np.concatenate([g["draws"], rs.randint(0, 2048, size=(n - len(g["draws"]), N, K))]).astype(np.int64)
    d0 = design_draws(rs, n, N, K, {1: t0, 3: t0})
    d2 = design_draws(rs, n, N, K, {0: t2})
    p0, p2 = synth.random_prompt(args, 8, 28, seed=41), synth.random_prompt(args, 7, 33, seed=42)
    prompts = [p0, (x1, xl1, y1), p2]
    eng = engine_for(args, sd, max_seqs=12, use_graph=graph)
    got = run_multi(eng, prompts, N, [d0, d1, d2], kn)
    assert np.array_equal(got[1], g["res"])
    assert eng.last_kept == [3, eng.last_kept[1], 0]
    orc = VoiceCraftOracle(args, sd)
    for u, d, t, j in ((0, d0, t0, 3), (2, d2, t2, 0)):
        want = oracle_best_of(orc, prompts[u], N, d, kn)
        assert got[u].shape == want.shape and np.array_equal(got[u], want), u
        check_kept(got[u], prompts[u], d, j, t)


def _repack_case():
    """Six utterances x 3 samples on a muted-terminator tiny model: utterances 1..5 terminate at steps 11..14 (1, 3 and 5 with
    simultaneous terminators), utterance 0 at step 70 - long after the batch was re-packed onto 4 rows (3 live + 1 filler)."""
    from voicecraft_amd import synth
    a = synth.make_args("tiny")
    sd = synth.make_state_dict(a, seed=6)
    K, N, n = a.n_codebooks, 3, 76
    prompts = [synth.random_prompt(a, 12, 20 + 3 * u, seed=60 + u) for u in range(6)]
    plan = [({0: 70, 2: 70}, 2, 70), ({1: 11, 2: 11}, 2, 11), ({0: 12}, 0, 12), ({0: 11, 1: 11, 2: 11}, 2, 11),
            ({1: 14}, 1, 14), ({0: 13, 1: 13}, 1, 13)]
    rs = np.random.RandomState(12)
    draws = [design_draws(rs, n, N, K, terms) for terms, _, _ in plan]
    return a, sd, prompts, draws, plan


def test_keep_decisions_after_repacks_next_to_filler_rows():
    from oracle.voicecraft_oracle import VoiceCraftOracle
    a, sd, prompts, draws, plan = _repack_case()
    kn = dict(top_k=0, top_p=1.0, temperature=1.0, stop_repetition=3)
    eng = engine_for(a, sd, max_seqs=18)
    res = {}
    for shrink in (1, 0):
        eng.set_option("shrink", shrink)
        res[shrink] = run_multi(eng, prompts, 3, draws, kn)
        assert eng.last_kept == [k for _, k, _ in plan], (shrink, eng.last_kept)
        assert (repacks(eng) >= 1) if shrink else (repacks(eng) == 0), (shrink, repacks(eng))
    for u in range(6):
        assert np.array_equal(res[1][u], res[0][u]), u
    orc = VoiceCraftOracle(a, sd)
    for u, (p, d, (_, k, t)) in enumerate(zip(prompts, draws, plan)):
        want = oracle_best_of(orc, p, 3, d, kn)
        assert res[1][u].shape == want.shape and np.array_equal(res[1][u], want), u
        check_kept(res[1][u], p, d, k, t)


def test_wide_steps_of_48_rows():
    """16 utterances x 3 samples = 48 rows: the first steps take the 17..64-row forms (census "wd")."""
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from voicecraft_amd import synth
    a = synth.make_args("tiny_h16")
    sd = synth.make_state_dict(a, seed=8)
    K, N, n = a.n_codebooks, 3, 24
    prompts = [synth.random_prompt(a, 6 + u % 4, 12 + u % 5, seed=300 + u) for u in range(16)]
    rs = np.random.RandomState(13)
    plan = [({0: 11 + u % 6, 2: 11 + u % 6}, 2) if u % 4 == 1 else ({u % 3: 11 + u % 6}, u % 3) for u in range(16)]
    draws = [design_draws(rs, n, N, K, terms) for terms, _ in plan]
    kn = dict(top_k=0, top_p=1.0, temperature=1.0, stop_repetition=3)
    eng = engine_for(a, sd, max_seqs=48)
    c0 = eng.launch_counts()
    got = run_multi(eng, prompts, N, draws, kn)
    c = {k: eng.launch_counts()[k] - c0[k] for k in c0}
    assert c["wd"] > 0, c
    assert eng.last_kept == [k for _, k in plan]
    orc = VoiceCraftOracle(a, sd)
    for u in range(0, 16, 4):
        want = oracle_best_of(orc, prompts[u], N, draws[u], kn)
        assert got[u].shape == want.shape and np.array_equal(got[u], want), u


def test_full_size_giga830M_bf16_batch_of_8_best_of_3():
    """BASELINE size in bf16: 8 utterances x 3 samples (24 rows), terminators on different steps.  Every utterance keeps the
    designed sample along its own draws; for two of them the oracle's replay gives the same tokens, and the head logits of every
    sample up to the terminator - and of the kept one after it - are within 2e-2 relative L2."""
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from voicecraft_amd import synth
    a = synth.make_args("giga830M")
    sd = synth.make_state_dict(a, seed=0, fast=True)
    K, N, n = a.n_codebooks, 3, 32
    prompts = [synth.random_prompt(a, 20 + 2 * u, 40 + 3 * u, seed=800 + u) for u in range(8)]
    plan = [({u % 3: 11 + 2 * u}, u % 3) if u % 2 else ({0: 11 + 2 * u, 1: 11 + 2 * u}, 1) for u in range(8)]
    rs = np.random.RandomState(14)
    draws = [design_draws(rs, n, N, K, terms) for terms, _ in plan]
    kn = dict(top_k=40, top_p=1.0, temperature=1.0, stop_repetition=3)
    steps = 11 + 2 * 7 + K
    eng = engine_for(a, sd, dtype="bf16", max_seqs=24)
    outs, lg = eng.inference_tts_multi([p[0][0] for p in prompts], [p[2][0] for p in prompts], **kn, batch_size=N,
                                       _forced=np.concatenate(draws, axis=1), _forced_mode="draws", _logit_steps=steps)
    got = [o[0].cpu().numpy() for o in outs]
    lg = lg.cpu().numpy()
    assert eng.last_kept == [k for _, k in plan]
    for u, (terms, k) in enumerate(plan):
        check_kept(got[u], prompts[u], draws[u], k, 11 + 2 * u)
    del eng
    torch.cuda.empty_cache()
    torch.set_num_threads(min(16, torch.get_num_threads() or 1) or 1)
    orc = VoiceCraftOracle(a, sd)
    for u in (0, 5):
        t, k = 11 + 2 * u, plan[u][1]
        trace = []
        want = oracle_best_of(orc, prompts[u], N, draws[u], kn, trace=trace)
        assert got[u].shape == want.shape and np.array_equal(got[u], want), u
        wl = torch.stack([tr["logits"] for tr in trace]).numpy()        # [steps][N][K][V]
        n_u = t + K
        for j in range(N):
            s1 = n_u if j == k else t + 1                                 # dropped samples stop at the terminator step
            rel = rel_l2(lg[:s1, u * N + j], wl[:s1, j])
            assert rel.max() <= 2e-2, (u, j, float(rel.max()))


def test_long_tts_best_of_3_in_chunks_of_two_sentences():
    """inference_tts_long(batch_size=3) on an engine of 8 sequences: five sentences in chunks of 8 // 3 = 2.  Greedy, with and
    without the shared-prefix reuse, every sentence equals an independent oracle inference_tts_batch(batch_size=3) on its
    full text; a draw replay through inference_tts_multi(_shared_text_prefix=P, batch_size=3) equals the oracle's; a later
    plain call is unaffected."""
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from voicecraft_amd import synth
    a = synth.make_args("tiny")
    sd = synth.make_state_dict(a, seed=21)
    rs = np.random.RandomState(8)
    x_prompt = torch.from_numpy(rs.randint(0, 100, size=(9,)).astype(np.int64))
    sents = [torch.from_numpy(rs.randint(0, 100, size=(n,)).astype(np.int64)) for n in (5, 11, 3, 8, 6)]
    _, _, y = synth.random_prompt(a, 1, 37, seed=9)
    eng = engine_for(a, sd, max_seqs=8, max_positions=512)
    orc = VoiceCraftOracle(a, sd)
    full = [torch.cat([x_prompt, sv]).unsqueeze(0) for sv in sents]
    greedy = dict(top_k=1, stop_repetition=3)
    want = [orc.inference_tts_batch(x, torch.tensor([x.shape[1]]), y, batch_size=3, **greedy)[0].numpy() for x in full]
    for reuse in (True, False):
        outs = eng.inference_tts_long(x_prompt, sents, y, **greedy, reuse_prefix=reuse, batch_size=3)
        assert len(outs) == len(sents) and len(eng.last_kept) == len(sents)
        for (res, gen), w in zip(outs, want):
            assert res.shape == w.shape and np.array_equal(res.cpu().numpy(), w), f"reuse={reuse}"
    # draw replay: sentences 0 and 1 with their transcript prefix shared
    K, N, n = a.n_codebooks, 3, 24
    prompts = [(x, torch.tensor([x.shape[1]]), y) for x in full[:2]]
    draws = [design_draws(rs, n, N, K, {1: 12}), design_draws(rs, n, N, K, {0: 15, 2: 15})]
    kn = dict(top_k=0, top_p=1.0, temperature=1.0, stop_repetition=3)
    got = run_multi(eng, prompts, N, draws, kn, _shared_text_prefix=int(x_prompt.numel()))
    assert eng.last_kept == [1, 2]
    for u in range(2):
        w = oracle_best_of(orc, prompts[u], N, draws[u], kn)
        assert got[u].shape == w.shape and np.array_equal(got[u], w), u
    x = full[1]
    single = orc.inference_tts(x, torch.tensor([x.shape[1]]), y, **greedy)[0].numpy()
    res = eng.inference_tts(x.cuda(), torch.tensor([x.shape[1]]).cuda(), y.cuda(), **greedy)[0]
    assert np.array_equal(res.cpu().numpy(), single)


@pytest.mark.parametrize("graph_steps", [2, 8])
def test_run_to_run_determinism_bf16(graph_steps):
    """Top-k 40 with live terminators, 6 utterances x 3 samples, bf16: four runs with the host disturbed differently before each
    give identical tokens, kept samples and re-pack counts (the width schedule follows the device, not the host's lag)."""
    from voicecraft_amd import synth
    a = synth.make_args("tiny128")
    # the live terminator of test_gpu_options.py's ragged batches, boosted less: a best-of-3 group keeps its EARLIEST terminator, and
    # at 0.45 every group ends within 11..14 frames; at 0.3 they spread over ~12..40.  Utterance 0's two-phoneme text caps it at 11
    # frames, so the batch re-packs while the others are still live
    sd = synth.make_state_dict(a, seed=4, mute_eos=False, boost=[(0, 2051, 0.3)])
    prompts = [synth.random_prompt(a, 2 if u == 0 else 8 + u, 9 + 2 * u, seed=900 + u) for u in range(6)]
    eng = engine_for(a, sd, dtype="bf16", max_seqs=18)
    eng.set_option("graph_steps", graph_steps)
    kn = dict(top_k=40, top_p=1.0, temperature=1.0, stop_repetition=3)
    junk = torch.randn(2048, 2048, device="cuda:0")

    def disturb(i):
        if i == 1:
            time.sleep(0.05)
        elif i == 2:
            for _ in range(20):
                junk.mul_(1.0001)                                      # queued device work ahead of the call
        elif i == 3:
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.02:                     # a busy host thread
                pass

    runs = []
    for i in range(4):
        disturb(i)
        outs = eng.inference_tts_multi([p[0][0] for p in prompts], [p[2][0] for p in prompts], **kn, batch_size=3, _seed=1234)
        runs.append(([o[0].cpu().numpy() for o in outs], list(eng.last_kept), repacks(eng)))
    assert runs[0][2] >= 1, runs[0][2]
    for r in runs[1:]:
        assert r[1] == runs[0][1] and r[2] == runs[0][2], (r[1:], runs[0][1:])
        for u in range(6):
            assert np.array_equal(r[0][u], runs[0][0][u]), u


def _one_utterance_calls(eng, name, N):
    g = load_golden(name)
    spec, args, sd, x, xl, y = build_case(name)
    kn = knobs_of(spec)
    got = run_multi(eng, [(x, xl, y)], N, [g["draws"]], kn)[0]
    assert np.array_equal(got, g["res"]), name
    return g, spec, x, xl, y


def test_one_utterance_is_unchanged():
    """inference_tts_multi([x], [y], batch_size=N) with the golden best-of draws gives the goldens; inference_tts_batch on the
    same engine still never re-packs (a call of one group keeps its N-row step)."""
    for name, N in (("tts_batch4_sampled", 4), ("tts_batch3_sampled_b", 3)):
        _, args, sd, _, _, _ = build_case(name)
        eng = engine_for(args, sd, max_seqs=8)
        g, spec, x, xl, y = _one_utterance_calls(eng, name, N)
        out = eng.inference_tts_batch(x.cuda(), xl.cuda(), y.cuda(), **spec["knobs"], _forced=g["draws"], _forced_mode="draws", _seed=3)
        assert np.array_equal(out[0].cpu().numpy(), g["res"])
        assert repacks(eng) == 0
        del eng


def test_validation():
    """batch_size 0, B*N > max_seqs and inference_tts_long(batch_size > max_seqs) are refused; the engine still gives the golden
    result afterwards."""
    name = "tts_batch4_sampled"
    spec, args, sd, x, xl, y = build_case(name)
    eng = engine_for(args, sd, max_seqs=8)
    xs, ys = [x[0], x[0]], [y[0], y[0]]
    with pytest.raises(AssertionError, match="batch_size"):
        eng.inference_tts_multi(xs, ys, top_k=1, batch_size=0)
    _one_utterance_calls(eng, name, 4)
    with pytest.raises(Exception, match="max_seqs"):
        eng.inference_tts_multi(xs + [x[0]], ys + [y[0]], top_k=1, batch_size=3)
    _one_utterance_calls(eng, name, 4)
    with pytest.raises(AssertionError, match="max_seqs"):
        eng.inference_tts_long(x[0, :3], [x[0, 3:]], y, top_k=1, batch_size=9)
    _one_utterance_calls(eng, name, 4)
