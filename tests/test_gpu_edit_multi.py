"""-m gpu: batched speech editing (vc_edit_multi / VoiceCraftEngine.inference_multi).

Every request of a batch must give what a single `inference` call gives (and what the reference / the oracle gives): a
span switch is fed over three one-row steps instead of vc_edit's one 3-row step, and those feed steps must leave no trace
in anything indexed by a request's sampled steps (gen rows, teacher forcing, draw replay, the logits hook, Philox).
"""
import numpy as np
import pytest
import torch

from _util import build_case, load_golden
from test_gpu_model import rel_l2

pytestmark = pytest.mark.gpu


def delta(after, before):
    return {k: after[k] - before[k] for k in after}


def engine_for(args, sd, dtype="fp32", **kw):
    from voicecraft_amd.engine import VoiceCraftEngine
    kw.setdefault("max_seqs", 8)
    kw.setdefault("max_positions", 512)
    return VoiceCraftEngine(args, sd, device="cuda:0", dtype=dtype, **kw)


def single(eng, x, y, spans, **kn):
    mi = torch.tensor([spans], dtype=torch.int64)
    return eng.inference(x.cuda(), torch.tensor([x.shape[1]]).cuda(), y.cuda(), mi, **kn).cpu().numpy()


def oracle_edit(orc, x, y, spans, **kn):
    mi = torch.tensor([spans], dtype=torch.int64)
    return orc.inference(x, torch.tensor([x.shape[1]]), y, mi, **kn).numpy()


GREEDY = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=-1)


@pytest.mark.parametrize("graph", [False, True])
def test_fp32_greedy_mixed_span_counts_in_one_call(graph):
    """The two golden prompts of the shared tiny model (edit_1span, edit_2span) in one batch with four more requests of 1, 2
    and 3 spans - among them edit_3span_edges' layout (a 1-frame head piece, the empty span (20, 20), a span to the end)."""
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from voicecraft_amd import synth
    s1, args, sd, x1, _, y1 = build_case("edit_1span")
    s2, _, _, x2, _, y2 = build_case("edit_2span")
    reqs = [(x1, y1, s1["spans"]), (x2, y2, s2["spans"])]
    for (Lx, T, seed), spans in [((9, 50, 501), [(1, 5), (20, 20), (44, 50)]), ((6, 40, 502), [(12, 19)]),
                                 ((10, 70, 503), [(5, 9), (30, 38)]), ((8, 45, 504), [(3, 4), (15, 22), (30, 31)])]:
        x, _, y = synth.random_prompt(args, Lx, T, seed=seed)
        reqs.append((x, y, spans))
    eng = engine_for(args, sd, use_graph=graph)
    outs = eng.inference_multi([r[0][0] for r in reqs], [r[1][0] for r in reqs], [r[2] for r in reqs], **GREEDY)
    assert len(outs) == len(reqs)
    assert np.array_equal(outs[0].cpu().numpy(), load_golden("edit_1span")["res"])
    assert np.array_equal(outs[1].cpu().numpy(), load_golden("edit_2span")["res"])
    orc = VoiceCraftOracle(args, sd)
    for (x, y, spans), got in zip(reqs[2:], outs[2:]):
        got = got.cpu().numpy()
        want = oracle_edit(orc, x, y, spans, **GREEDY)
        assert got.shape == want.shape and np.array_equal(got, want), spans
        assert np.array_equal(got, single(eng, x, y, spans, **GREEDY)), spans


def test_fp32_draw_replay_with_switches_on_different_steps():
    """Sampled editing (unmuted terminator): request 0 replays the reference's recorded draws and must give the golden; requests
    1 and 2 replay hand-made draws whose terminators put their span switches on different steps, one of them on the step where
    request 0 retires.  Both must equal the oracle replaying the same draws."""
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from voicecraft_amd import synth
    spec, args, sd, x0, _, y0 = build_case("edit_sampled_eog")
    g = load_golden("edit_sampled_eog")
    kn = dict(spec["knobs"])
    kn.pop("kvcache")
    K = args.n_codebooks
    eng = engine_for(args, sd, max_seqs=4)
    d0 = np.asarray(g["draws"]).reshape(-1, K)
    got0 = eng.inference_multi([x0[0]], [y0[0]], [spec["spans"]], **kn, _forced=d0[:, None], _forced_mode="draws", _seed=99)
    assert np.array_equal(got0[0].cpu().numpy(), g["res"])
    last0 = eng.last_steps                      # sampled steps of request 0; it retires on batch step last0 - 1 + 2 (one switch)
    n = 160
    rs = np.random.RandomState(17)
    draws = rs.randint(0, 2048, size=(n, 3, K)).astype(np.int64)
    draws[: len(d0), 0] = d0
    p1 = max(1, last0 + 2 - K)                   # request 1: its first span ends on that batch step (p1 + K - 1)
    for b, (p, q) in ((1, (p1, p1 + 20)), (2, (5, 40))):
        draws[:, b, 0] = np.where(draws[:, b, 0] == args.eog, 7, draws[:, b, 0])
        draws[p, b, 0] = args.eog
        draws[q::12, b, 0] = args.eog            # (the second span ends on the first of these after it starts)
    reqs = [(x0, y0, spec["spans"])]
    for Lx, T, seed, spans in ((20, 60, 601, [(12, 20), (30, 41)]), (22, 64, 602, [(8, 16), (40, 50)])):
        x, _, y = synth.random_prompt(args, Lx, T, seed=seed)
        reqs.append((x, y, spans))
    outs = eng.inference_multi([r[0][0] for r in reqs], [r[1][0] for r in reqs], [r[2] for r in reqs], **kn,
                               _forced=draws, _forced_mode="draws", _seed=5)
    assert np.array_equal(outs[0].cpu().numpy(), g["res"])
    orc = VoiceCraftOracle(args, sd)
    for b in (1, 2):
        x, y, spans = reqs[b]
        want = orc.inference(x, torch.tensor([x.shape[1]]), y, torch.tensor([spans]), **kn, forced_draws=draws[:, b]).numpy()
        got = outs[b].cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), b


def test_fp32_old_special_token_scheme():
    """edit_oldscheme (eos = -1, every piece closed by eog) in a batch with oracle-checked companions of 2 and 3 spans."""
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from voicecraft_amd import synth
    spec, args, sd, x0, _, y0 = build_case("edit_oldscheme")
    reqs = [(x0, y0, spec["spans"])]
    for Lx, T, seed, spans in ((7, 48, 701, [(6, 12), (30, 35)]), (9, 52, 702, [(2, 6), (20, 20), (40, 52)])):
        x, _, y = synth.random_prompt(args, Lx, T, seed=seed)
        reqs.append((x, y, spans))
    eng = engine_for(args, sd, max_seqs=4)
    outs = eng.inference_multi([r[0][0] for r in reqs], [r[1][0] for r in reqs], [r[2] for r in reqs], **GREEDY)
    assert np.array_equal(outs[0].cpu().numpy(), load_golden("edit_oldscheme")["res"])
    orc = VoiceCraftOracle(args, sd)
    for (x, y, spans), got in zip(reqs[1:], outs[1:]):
        want = oracle_edit(orc, x, y, spans, **GREEDY)
        assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want), spans


def test_one_decode_row_per_request():
    """8 two-span requests: every decode step runs one row per request (8-row finished-row forms), never a 17..64-row form; a
    3-row switch layout would have run 24 rows on one."""
    from voicecraft_amd import synth
    args = synth.make_args("tiny")
    sd = synth.make_state_dict(args, seed=3)
    reqs = []
    for u in range(8):
        x, _, y = synth.random_prompt(args, 6 + u % 3, 40 + 2 * u, seed=800 + u)
        reqs.append((x, y, [(4 + u % 3, 10 + u % 4), (20, 26 + u % 5)]))
    eng = engine_for(args, sd)
    c0 = eng.launch_counts()
    outs = eng.inference_multi([r[0][0] for r in reqs], [r[1][0] for r in reqs], [r[2] for r in reqs], **GREEDY)
    c = delta(eng.launch_counts(), c0)
    assert c["wd"] == 0 and c["mt2"] == 0 and c["mt4"] == 0, c
    assert c["rows_gemm_fr"] + c["rows_gemm_frp"] > 0, c
    for (x, y, spans), got in zip(reqs[:2], outs[:2]):
        assert np.array_equal(got.cpu().numpy(), single(eng, x, y, spans, **GREEDY))


def test_wide_batch_and_shrinking():
    """24 requests on the 16-head model (17..64-row steps): fp32 greedy against the oracle for every third request.  Then a
    ragged batch of 12 with shrink on and off: identical tokens, and the batch re-packs only with shrink on."""
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from voicecraft_amd import synth
    a = synth.make_args("tiny_h16")
    sd = synth.make_state_dict(a, seed=4)
    reqs = []
    for u in range(24):
        x, _, y = synth.random_prompt(a, 4 + (u % 5), 20 + 3 * (u % 7), seed=900 + u)
        spans = [(3, 7)] if u % 2 == 0 else [(2, 5), (10, 14)]
        reqs.append((x, y, spans))
    eng = engine_for(a, sd, max_seqs=24, max_positions=256)
    outs = eng.inference_multi([r[0][0] for r in reqs], [r[1][0] for r in reqs], [r[2] for r in reqs], **GREEDY)
    orc = VoiceCraftOracle(a, sd)
    for u in range(0, 24, 3):
        x, y, spans = reqs[u]
        want = oracle_edit(orc, x, y, spans, **GREEDY)
        got = outs[u].cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), u
    rag = []
    for u in range(12):
        x, _, y = synth.random_prompt(a, 3 + u, 24 + u, seed=950 + u)
        rag.append((x, y, [(4, 8), (12, 15)] if u % 3 else [(5, 9)]))
    res = {}
    for shrink in (1, 0):
        eng.set_option("shrink", shrink)
        o = eng.inference_multi([r[0][0] for r in rag], [r[1][0] for r in rag], [r[2] for r in rag], **GREEDY)
        res[shrink] = ([t.cpu().numpy() for t in o], float(eng.debug_read("host_ms", (8,), torch.float64)[6]))
    eng.set_option("shrink", 1)
    assert all(np.array_equal(p, q) for p, q in zip(res[1][0], res[0][0]))
    assert res[1][1] >= 1 and res[0][1] == 0, (res[1][1], res[0][1])


def test_baseline_size_bf16_eight_c4_requests():
    """BASELINE config 4's shape, eight requests at giga830M, bf16, teacher-forced: the logits of two requests at steps 0, 40
    and n-1 within 2e-2 relative L2 of the oracle's one-pass evaluation, on 8-row steps.  Then, in fp32, a 2-span giga request
    inside a batch takes the feed-step path and must give the oracle's greedy tokens."""
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from test_gpu_scale import forced_trajectory
    from voicecraft_amd import synth
    a = synth.make_args("giga830M")
    sd = synth.make_state_dict(a, seed=0, fast=True)
    torch.set_num_threads(min(16, torch.get_num_threads() or 1) or 1)
    orc = VoiceCraftOracle(a, sd)
    B, n = 8, 80
    reqs = []
    for u in range(B):
        x, _, y = synth.random_prompt(a, 80, 800, seed=1 + u)
        reqs.append((x, y, [(300 + 4 * u, 400 + 2 * u)]))
    forced = np.stack([forced_trajectory(a, n, seed=4 + u, term=a.eog) for u in range(B)], axis=1)     # [n,B,K]
    steps = [0, 40, n - 1]
    eng = engine_for(a, sd, dtype="bf16", max_seqs=B, max_positions=1024)
    c0 = eng.launch_counts()
    outs, lg = eng.inference_multi([r[0][0] for r in reqs], [r[1][0] for r in reqs], [r[2] for r in reqs], top_k=40,
                                   _forced=forced, _logit_steps=n)
    c = delta(eng.launch_counts(), c0)
    assert c["wd"] == 0 and c["mt2"] == 0 and c["rows_gemm_fr"] + c["rows_gemm_frp"] > 0, c
    lg = lg.cpu().numpy()
    for u in (0, 5):
        x, y, spans = reqs[u]
        s0, s1 = spans[0]
        assert outs[u].shape == (1, a.n_codebooks, 800 - (s1 - s0) + (n - a.n_codebooks))
        want = orc.edit_logits_for_trajectory(x, y, torch.tensor([spans]), forced[:, u], steps=steps).numpy()
        rel = rel_l2(lg[steps, u], want)
        assert rel.max() <= 2e-2, (u, dict(zip(steps, rel.tolist())))
    del eng
    torch.cuda.empty_cache()
    x, xl, y = synth.random_prompt(a, 5, 30, seed=41)
    spans = [(5, 10), (18, 24)]
    want = oracle_edit(orc, x, y, spans, top_k=1, stop_repetition=3)
    x2, _, y2 = synth.random_prompt(a, 6, 28, seed=42)
    e32 = engine_for(a, sd, dtype="fp32", max_seqs=2, max_positions=256)
    outs = e32.inference_multi([x[0], x2[0]], [y[0], y2[0]], [spans, [(4, 9)]], top_k=1, stop_repetition=3)
    got = outs[0].cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("name", ["edit_2span", "edit_3span_edges"])
def test_single_request_through_the_batched_entry(name):
    """B = 1: the feed-step path alone must reproduce the multi-span goldens exactly."""
    spec, args, sd, x, _, y = build_case(name)
    eng = engine_for(args, sd, max_seqs=2)
    out = eng.inference_multi([x[0]], [y[0]], [torch.tensor([spec["spans"]])], **GREEDY)
    assert len(out) == 1 and np.array_equal(out[0].cpu().numpy(), load_golden(name)["res"])


def test_validation_names_the_request_and_leaves_the_engine_usable():
    from voicecraft_amd._lib import EngineError
    spec, args, sd, x, _, y = build_case("edit_2span")
    g = load_golden("edit_2span")["res"]
    eng = engine_for(args, sd, max_seqs=3)
    xs, ys = [x[0]] * 3, [y[0]] * 3
    ok = spec["spans"]
    with pytest.raises(AssertionError, match="request 2: mask interval 0 is reversed"):
        eng.inference_multi(xs, ys, [ok, ok, [(30, 20)]], **GREEDY)
    with pytest.raises(IndexError, match="request 1"):
        eng.inference_multi(xs, ys, [ok, [(0, 3)], ok], **GREEDY)
    with pytest.raises(AssertionError, match="request 0"):
        eng.inference_multi(xs, ys, [[(2, 3), (5, 6), (8, 9), (12, 14)], ok, ok], **GREEDY)     # 4 spans, max_n_spans 3
    with pytest.raises(EngineError, match="max_seqs"):
        eng.inference_multi([x[0]] * 4, [y[0]] * 4, [ok] * 4, **GREEDY)
    out = eng.inference_multi(xs, ys, [ok] * 3, **GREEDY)
    assert all(np.array_equal(o.cpu().numpy(), g) for o in out)
