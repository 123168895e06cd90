"""-m gpu: editing requests and per-request sampling controls in a decode session (include/vc_engine.h vc_session_submit_ctl,
vc_session_submit_edit).  TTS and editing requests with different controls share one decode step; every request must still be its
own blocking call: in exact mode equal to the oracle's run of that request alone (`inference_tts` / `inference`), with sampling
bit-equal to the one-row-per-request blocking call with its seed and controls.  Every comparison is bit equality of token ids."""
import time

import numpy as np
import pytest
import torch

from _util import build_case, load_golden

pytestmark = pytest.mark.gpu

GREEDY_TTS = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=3)
GREEDY_EDIT = dict(top_k=1, top_p=1.0, temperature=1.0, stop_repetition=-1)


# ------------------------------------------------------------------------------------------------ requests, schedules
def tts_req(x, xl, y, seed=None, **controls):
    return dict(kind="tts", x=x, xl=xl, y=y, spans=None, seed=seed, controls=controls)


def edit_req(x, xl, y, spans, seed=None, **controls):
    return dict(kind="edit", x=x, xl=xl, y=y, spans=[tuple(s) for s in spans], seed=seed, controls=controls)


def submit(sess, r):
    if r["kind"] == "tts":
        return sess.submit(r["x"], r["xl"], r["y"], seed=r["seed"], **r["controls"])
    return sess.submit_edit(r["x"], r["xl"], r["y"], torch.tensor([r["spans"]], dtype=torch.int64), seed=r["seed"], **r["controls"])


def run_schedule(eng, max_live, reqs, schedule, **open_kw):
    """schedule: ("submit", lo, hi) / ("poll", n) operations; afterwards the session is polled until idle.
    Returns (results by request index as numpy, the request indices each poll reported, stats)."""
    tickets, polls, done = {}, [], {}
    with eng.open_session(max_live, **open_kw) as sess:
        def poll():
            got = sess.poll()
            polls.append([tickets[t] for t, _, _ in got])
            for t, res, gen in got:
                u = tickets[t]
                assert (gen is None) == (reqs[u]["kind"] == "edit"), (u, reqs[u]["kind"])
                done[u] = res.cpu().numpy()
        for op in schedule:
            if op[0] == "submit":
                for u in range(op[1], op[2]):
                    tickets[submit(sess, reqs[u])] = u
            else:
                for _ in range(op[1]):
                    poll()
        while not sess.idle:
            poll()
        stats = sess.stats()
    assert sorted(done) == list(range(len(reqs))), sorted(done)
    return [done[u] for u in range(len(reqs))], polls, stats


def oracle_run(orc, r, trace=None, **kn):
    """The oracle's own run of one request (greedy unless told otherwise): res as numpy."""
    if r["kind"] == "tts":
        kn = {**GREEDY_TTS, **kn}
        return orc.inference_tts(r["x"], r["xl"], r["y"], trace=trace, **kn)[0].numpy()
    kn = {**GREEDY_EDIT, **kn}
    return orc.inference(r["x"], r["xl"], r["y"], torch.tensor([r["spans"]], dtype=torch.int64), trace=trace, **kn).numpy()


def span_steps(trace, term, K):
    """Sampled steps of each finished span of an oracle run: a span ends on the step whose last codebook emits the terminator."""
    out, n = [], 0
    for t in trace:
        n += 1
        if int(t["tokens"][K - 1]) == term:
            out.append(n)
            n = 0
    assert n == 0, "the oracle's run ended inside a span"
    return out


def row_actions(steps):
    """What a request's decode row does, row step by row step: 'S' a sampled step, 'F' a fed row of a span switch (two per switch:
    the mask_embedding row and the all-empty column; the switch's first row is the input the span's last sampled step left)."""
    acts = []
    for i, n in enumerate(steps):
        acts += ["S"] * n + (["F", "F"] if i + 1 < len(steps) else [])
    return acts


def simulate(actions, schedule, max_live, G, top=None):
    """The session's host logic replayed on the CPU (vc_engine_session.hip vc_session_advance; DecodeSession.poll fetches what a turn reports
    and so frees those slots for the NEXT turn).  A request admitted in front of batch a takes row step 0 (its first sample) there and
    row step j >= 1 in batch a + (j - 1) // G; it retires in the batch of its last row step, and the host counts that once it has seen
    that batch end (two batches may be in flight).  Returns the counters of DecodeSession.stats(), the request indices each poll
    reports, and `mid_switch`: (admitted request, live edit) pairs where the edit had fed some but not all rows of a span switch."""
    def width_for(n):
        p = 1
        while p < n:
            p *= 2
        return p
    top = width_for(max_live) if top is None else top
    n = len(actions)
    fifo, slots = [], [None] * max_live
    state, adm, ret = ["new"] * n, [None] * n, [None] * n
    c = dict(admitted=0, admitted_while_live=0, turns=0, widenings=0, narrowings=0, live_rows=0, launched_rows=0)
    S = dict(batch=0, run_start=0, live=0, B=0, idle=True)
    polls, mid_switch = [], []

    def note(known, fin):
        for s, u in enumerate(slots):
            if u is not None and state[u] == "live" and ret[u] <= known:
                state[u] = "finished"
                S["live"] -= 1
                c["live_rows"] += len(actions[u]) - 1
                fin.append(u)

    def advance():
        c["turns"] += 1
        fin = []
        known = S["batch"] - 2 if S["batch"] - S["run_start"] >= 2 else S["run_start"] - 1
        note(known, fin)
        live_before, new = S["live"], []
        for s in range(max_live):
            if slots[s] is None and fifo:
                u = fifo.pop(0)
                slots[s], state[u] = u, "live"
                new.append(u)
        if S["live"] + len(new) == 0:
            if S["batch"] > S["run_start"]:
                note(S["batch"] - 1, fin)
                S["run_start"] = S["batch"]
            S["idle"] = not fifo
        else:
            b = S["batch"]
            w = min(width_for(max(1, S["live"] + len(new))), top)
            c["widenings"] += int(S["B"] > 0 and w > S["B"])
            c["narrowings"] += int(w < S["B"])
            S["B"] = w
            for u in new:
                for v in range(n):          # edits on the device right now, between the first and the last row of a switch
                    if adm[v] is not None and v != u and state[v] != "new":
                        nxt = 1 + (b - adm[v]) * G
                        if nxt < len(actions[v]) and actions[v][nxt] == "F":
                            mid_switch.append((u, v))
                adm[u] = b
                last = len(actions[u]) - 1
                ret[u] = b + (last - 1) // G if last >= 1 else b
            c["admitted"] += len(new)
            c["admitted_while_live"] += len(new) if live_before > 0 else 0
            S["live"] += len(new)
            S["batch"] += 1
            c["launched_rows"] += w * G
        polls.append(fin)
        for u in fin:                       # DecodeSession._turn fetches everything the turn reported
            slots[slots.index(u)] = None
            state[u] = "fetched"

    for op in schedule:
        if op[0] == "submit":
            fifo += list(range(op[1], op[2]))
            S["idle"] = False
        else:
            for _ in range(op[1]):
                advance()
    while not S["idle"]:
        advance()
    return c, polls, mid_switch


def engine_for(args, sd, dtype="fp32", **kw):
    from voicecraft_amd.engine import VoiceCraftEngine
    kw.setdefault("max_seqs", 4)
    kw.setdefault("max_positions", 512)
    return VoiceCraftEngine(args, sd, device="cuda:0", dtype=dtype, **kw)


# ------------------------------------------------------------------------------------------------ 1. three goldens, one session
@pytest.mark.parametrize("graph", [True, False])
def test_three_goldens_share_one_session(graph):
    """tts_greedy, edit_1span and edit_2span (one model; stop_repetition 3 against -1) through one session opened with other
    defaults (top_k 40): each equals its golden.  Their sampled steps are 43, 24 and 33 (+ 2 fed rows for the two-span edit), so
    with 4 steps per batch they retire in batches 10, 5 and 8 and are reported by three different turns, shortest first."""
    s0, args, sd, x0, xl0, y0 = build_case("tts_greedy")
    s1, _, _, x1, xl1, y1 = build_case("edit_1span")
    s2, _, _, x2, xl2, y2 = build_case("edit_2span")
    reqs = [tts_req(x0, xl0, y0, top_k=1, stop_repetition=3),
            edit_req(x1, xl1, y1, s1["spans"], top_k=1, stop_repetition=-1),
            edit_req(x2, xl2, y2, s2["spans"], top_k=1, stop_repetition=-1)]
    eng = engine_for(args, sd, use_graph=graph)
    eng.set_option("graph_steps", 4)
    got, polls, stats = run_schedule(eng, 3, reqs, [("submit", 0, 3)], top_k=40, stop_repetition=3)
    for u, name in enumerate(("tts_greedy", "edit_1span", "edit_2span")):
        want = load_golden(name)["res"]
        assert got[u].shape == tuple(want.shape) and np.array_equal(got[u], want), name
    order = [p for p in polls if p]
    assert order == [[1], [2], [0]], polls
    # (how the two-span edit's 33 steps split over its spans does not enter the counters: only its 33 + 2 row steps do)
    sim, sim_polls, _ = simulate([row_actions([43]), row_actions([24]), row_actions([29, 4])], [("submit", 0, 3)], 3, 4)
    assert [p for p in sim_polls if p] == order and {k: stats[k] for k in sim} == sim, (stats, sim)


# ------------------------------------------------------------------------------------------------ 2. mixed, ragged, refilled
# submit 2, poll four turns, submit 4 more, poll twice, submit the rest; 2 steps per batch.  With the oracle's step counts this admits
# request 9 in front of the batch in which request 5 (the 3-span edit) feeds the second row of a span switch (check_mixed_inputs)
MIXED_SCHEDULE = [("submit", 0, 2), ("poll", 4), ("submit", 2, 6), ("poll", 2), ("submit", 6, 14)]
MIXED_G = 2
_MIXED = {}


def mixed_requests():
    """14 requests on the model of tts_greedy, 7 of them edits of 1, 2 and 3 spans; request 5 has edit_3span_edges' layout (a
    1-frame head piece, an empty span, a span to the end).  Expected values: each request's own greedy oracle run, once."""
    if _MIXED:
        return _MIXED["v"]
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from voicecraft_amd import synth
    _, args, sd, _, _, _ = build_case("tts_greedy")
    shapes = [("tts", 6, 21, None), ("edit", 9, 64, [(10, 18), (40, 47)]), ("tts", 3, 12, None), ("edit", 8, 60, [(20, 31)]),
              ("tts", 7, 40, None), ("edit", 9, 50, [(1, 5), (20, 20), (44, 50)]), ("edit", 7, 44, [(5, 9), (30, 38)]),
              ("tts", 4, 9, None), ("edit", 6, 40, [(12, 19)]), ("tts", 5, 33, None), ("edit", 8, 45, [(3, 4), (15, 22), (30, 31)]),
              ("tts", 8, 27, None), ("edit", 10, 70, [(5, 9), (30, 38)]), ("tts", 4, 30, None)]
    reqs = []
    for u, (kind, Lx, T, spans) in enumerate(shapes):
        x, xl, y = synth.random_prompt(args, Lx, T, seed=1200 + u)
        reqs.append(tts_req(x, xl, y, **GREEDY_TTS) if kind == "tts" else edit_req(x, xl, y, spans, **GREEDY_EDIT))
    torch.set_num_threads(min(4, torch.get_num_threads()))
    orc = VoiceCraftOracle(args, sd)
    want, steps = [], []
    for r in reqs:
        trace = []
        want.append(oracle_run(orc, r, trace=trace))
        term = args.eog if r["kind"] == "edit" else (args.eos if args.eos > 0 else args.eog)
        steps.append(span_steps(trace, term, args.n_codebooks))
    _MIXED["v"] = (args, sd, reqs, want, steps)
    return _MIXED["v"]


def check_mixed_inputs(args, reqs, want, steps):
    """The conditions the schedule is chosen for, from the oracle's results alone."""
    K = args.n_codebooks
    for r, w, st in zip(reqs, want, steps):
        if r["kind"] == "edit":
            assert len(st) == len(r["spans"]) and max(st) > K, (r["spans"], st)      # a span of more than K steps holds a frame
            kept = r["y"].shape[1] - sum(e - s for s, e in r["spans"])
            assert w.shape[2] == kept + sum(n - K for n in st), (w.shape, kept, st)
    totals = [sum(st) for st in steps]
    assert min(totals) * 2 <= max(totals), totals
    sim, polls, mid = simulate([row_actions(st) for st in steps], MIXED_SCHEDULE, 4, MIXED_G)
    assert mid, "no request is admitted while an edit is inside a span switch: choose another schedule"
    assert all(reqs[v]["kind"] == "edit" for _, v in mid)
    return sim, polls


def test_mixed_ragged_refilled_fp32():
    args, sd, reqs, want, steps = mixed_requests()
    sim, sim_polls = check_mixed_inputs(args, reqs, want, steps)
    eng = engine_for(args, sd)
    eng.set_option("graph_steps", MIXED_G)
    runs = [run_schedule(eng, 4, reqs, MIXED_SCHEDULE, top_k=40, stop_repetition=3) for _ in range(2)]
    for got, polls, stats in runs:
        print(stats)
        assert stats["admitted"] == len(reqs) and stats["admitted_while_live"] >= 1, stats
        assert 0 < stats["live_rows"] <= stats["launched_rows"], stats
    assert runs[0][2] == runs[1][2] and runs[0][1] == runs[1][1], (runs[0][2], runs[1][2])
    # the schedule the input conditions were derived for is the schedule that ran
    assert {k: runs[0][2][k] for k in sim} == sim and runs[0][1] == sim_polls, (runs[0][2], sim)
    for got, _, _ in runs:
        for u, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and np.array_equal(g, w), (u, reqs[u]["kind"], reqs[u]["spans"], g.shape, w.shape)


# ------------------------------------------------------------------------------------------------ 3. other token shapes
@pytest.mark.parametrize("edit_name,tts_prompt", [("edit_k8_2span", (5, 17, 41)), ("edit_oldscheme", (6, 19, 14))])
def test_other_token_shapes(edit_name, tts_prompt):
    """K = 8, and the old special-token scheme (eos = -1: every piece closed by eog), each through a 2-slot session next to one TTS
    request of its model: the edit equals its golden, the TTS request its own oracle run."""
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from voicecraft_amd import synth
    spec, args, sd, x, xl, y = build_case(edit_name)
    kn = {k: v for k, v in spec["knobs"].items() if k != "kvcache"}
    xt, xlt, yt = synth.random_prompt(args, *tts_prompt[:2], seed=tts_prompt[2])
    reqs = [tts_req(xt, xlt, yt, **GREEDY_TTS), edit_req(x, xl, y, spec["spans"], **kn)]
    eng = engine_for(args, sd, max_seqs=2)
    got, _, stats = run_schedule(eng, 2, reqs, [("submit", 0, 2)], top_k=40)
    want = load_golden(edit_name)["res"]
    assert got[1].shape == tuple(want.shape) and np.array_equal(got[1], want)
    w0 = oracle_run(VoiceCraftOracle(args, sd), reqs[0])
    assert got[0].shape == w0.shape and np.array_equal(got[0], w0)
    assert stats["admitted"] == 2


# ------------------------------------------------------------------------------------------------ 4. wide steps
def test_wide_steps_tts_and_edits():
    """tiny_h16, 20 slots: 24 requests, every third a two-span edit, through the 17..64-row step forms with admissions and a change
    of width on the way.  Every request equals its own oracle run (the TTS ones share test_gpu_session.py's cached runs)."""
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from test_gpu_session import _oracle, _workload
    from voicecraft_amd import synth
    a, sd, prompts = _workload("tiny_h16", 16)
    want_tts = _oracle("tiny_h16", 16)
    torch.set_num_threads(min(4, torch.get_num_threads()))
    orc = VoiceCraftOracle(a, sd)
    reqs, want = [], []
    it = iter(range(16))
    for u in range(24):
        if u % 3 == 2:
            x, xl, y = synth.random_prompt(a, 4 + (u % 5), 20 + 3 * (u % 7), seed=1300 + u)
            reqs.append(edit_req(x, xl, y, [(2, 5), (10, 14)], **GREEDY_EDIT))
            want.append(oracle_run(orc, reqs[-1]))
        else:
            i = next(it)
            reqs.append(tts_req(*prompts[i], **GREEDY_TTS))
            want.append(want_tts[i])
    eng = engine_for(a, sd, max_seqs=20, max_positions=256)
    got, _, stats = run_schedule(eng, 20, reqs, [("submit", 0, 24)], top_k=40)
    print(stats)
    for u, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (u, reqs[u]["kind"])
    assert stats["admitted"] == 24 and stats["widenings"] + stats["narrowings"] >= 1, stats
    assert 0 < stats["live_rows"] <= stats["launched_rows"], stats


# ------------------------------------------------------------------------------------------------ 5. one slot = the blocking call
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_one_slot_is_the_blocking_call(dtype):
    """max_live = 1, sampled, live terminators (edit_sampled_eog's model): a TTS request, a two-span edit with controls of its own
    and another TTS request go through the one slot; each is bit-equal to the blocking one-row-per-request call with its seed and
    controls on the same engine (inference_tts; inference_multi of one request - both decode one row with fed switches)."""
    from voicecraft_amd import synth
    spec, args, sd, xe, xle, ye = build_case("edit_sampled_eog")
    ekn = {k: v for k, v in spec["knobs"].items() if k != "kvcache"}          # top_k 30, top_p 0.8, stop_repetition 2
    tkn = dict(top_k=40, top_p=1.0, temperature=1.0, stop_repetition=3)
    p0, p2 = synth.random_prompt(args, 6, 21, seed=1401), synth.random_prompt(args, 5, 14, seed=1402)
    eng = engine_for(args, sd, dtype, max_seqs=1)
    want = [eng.inference_tts(p0[0].cuda(), p0[1].cuda(), p0[2].cuda(), **tkn, _seed=11)[0].cpu().numpy(),
            eng.inference_multi([xe[0]], [ye[0]], [spec["spans"]], **ekn, _seed=12)[0].cpu().numpy(),
            eng.inference_tts(p2[0].cuda(), p2[1].cuda(), p2[2].cuda(), **tkn, _seed=13)[0].cpu().numpy()]
    reqs = [tts_req(*p0, seed=11), edit_req(xe, xle, ye, spec["spans"], seed=12, **ekn), tts_req(*p2, seed=13)]
    got, _, stats = run_schedule(eng, 1, reqs, [("submit", 0, 3)], **tkn)
    for u, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (dtype, u, g.shape, w.shape)
    assert stats["admitted"] == 3 and stats["admitted_while_live"] == 0 and stats["widenings"] == stats["narrowings"] == 0, stats
    # and the blocking calls are untouched by the session before them
    again = eng.inference_multi([xe[0]], [ye[0]], [spec["spans"]], **ekn, _seed=12)[0].cpu().numpy()
    assert np.array_equal(again, want[1])


# ------------------------------------------------------------------------------------------------ 6. controls do not leak
def test_controls_do_not_leak_between_rows():
    """Request B (sampled: top_k 40, temperature 0.8, fixed seed) decodes next to request A, same schedule twice.  Run 1: A greedy.
    Run 2: A with top_p 0.5, temperature 1.3, stop_repetition 1 and another seed.  B's tokens are the same in both runs; run 1's A
    equals its greedy oracle run."""
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from voicecraft_amd import synth
    spec, args, sd, _, _, _ = build_case("edit_sampled_eog")
    xa, xla, ya = synth.random_prompt(args, 7, 30, seed=1501)
    xb, xlb, yb = synth.random_prompt(args, 8, 60, seed=1502)
    b = edit_req(xb, xlb, yb, [(12, 20), (30, 41)], seed=77, top_k=40, temperature=0.8)
    a1 = tts_req(xa, xla, ya, seed=5, top_k=1)
    a2 = tts_req(xa, xla, ya, seed=6, top_p=0.5, temperature=1.3, stop_repetition=1)
    eng = engine_for(args, sd, max_seqs=2)
    eng.set_option("graph_steps", 4)
    open_kw = dict(top_k=-100, top_p=1.0, temperature=1.0, stop_repetition=3)
    run1, _, st1 = run_schedule(eng, 2, [a1, b], [("submit", 0, 2)], **open_kw)
    run2, _, st2 = run_schedule(eng, 2, [a2, b], [("submit", 0, 2)], **open_kw)
    assert run1[1].shape == run2[1].shape and np.array_equal(run1[1], run2[1])
    wa = oracle_run(VoiceCraftOracle(args, sd), a1)
    assert run1[0].shape == wa.shape and np.array_equal(run1[0], wa)
    assert not (run1[0].shape == run2[0].shape and np.array_equal(run1[0], run2[0])), "A's controls changed nothing: the test shows nothing"
    # B sampled for real: its greedy run differs
    g = run_schedule(eng, 2, [a1, {**b, "controls": dict(top_k=1)}], [("submit", 0, 2)], **open_kw)[0][1]
    assert not (g.shape == run1[1].shape and np.array_equal(g, run1[1]))


# ------------------------------------------------------------------------------------------------ 7. bf16 determinism
def test_mixed_schedule_bf16_sampled_is_the_same_in_every_run():
    """The mixed schedule in bf16, sampled with top-k 40: three runs, the host disturbed differently before each - same tokens, same
    counters, same order of results."""
    args, sd, reqs, _, _ = mixed_requests()
    seeded = [{**r, "seed": 300 + u, "controls": {}} for u, r in enumerate(reqs)]      # (the session's controls: sampled)
    eng = engine_for(args, sd, "bf16")
    eng.set_option("graph_steps", MIXED_G)
    runs = []
    for i in range(3):
        if i:
            time.sleep(0.02 * i)                      # another phase between the host's loop and the device's
        runs.append(run_schedule(eng, 4, seeded, MIXED_SCHEDULE, top_k=40, stop_repetition=3))
    assert runs[0][2]["admitted_while_live"] >= 1, runs[0][2]
    for got, polls, stats in runs[1:]:
        assert stats == runs[0][2] and polls == runs[0][1], (stats, runs[0][2])
        for u, (g, w) in enumerate(zip(got, runs[0][0])):
            assert g.shape == w.shape and np.array_equal(g, w), u


# ------------------------------------------------------------------------------------------------ 8. refusals; failures stay local
def _drain_collecting_failures(sess):
    from voicecraft_amd.engine import SessionRequestError
    failed = {}
    for _ in range(64):
        try:
            return sess.drain(), failed
        except SessionRequestError as ex:
            failed.update(ex.failed)
    raise AssertionError("the session did not drain")


def test_refused_edits_leave_the_session_running():
    from voicecraft_amd import synth
    from voicecraft_amd._lib import EngineError
    spec, args, sd, x, xl, y = build_case("edit_2span")
    g2 = load_golden("edit_2span")["res"]
    eng = engine_for(args, sd)
    mi = lambda spans: torch.tensor([spans], dtype=torch.int64)
    with pytest.raises(AssertionError, match="not supported"):
        eng.open_session(2, batch_size=3)
    with eng.open_session(2, top_k=40, stop_repetition=3) as sess:
        # each refusal carries the message `inference` gives for the same input
        bad = [(mi([(30, 20)]), AssertionError, "mask interval 0 is reversed"),
               (mi([(10, 30), (20, 40)]), IndexError, "zero-length non-masked piece"),      # overlap: a piece of negative length
               (mi([(0, 3)]), IndexError, "zero-length non-masked piece"),
               (mi([(2, 3), (5, 6), (8, 9), (12, 14)]), AssertionError, "4 spans but max_n_spans is 3")]
        for m, exc, msg in bad:
            with pytest.raises(exc, match=msg):
                sess.submit_edit(x, xl, y, m, **GREEDY_EDIT)
        xl_, xll_, yl_ = synth.random_prompt(args, 8, 520, seed=3)      # the rearranged prompt alone exceeds max_positions (512)
        with pytest.raises(EngineError, match="rearranged prompt alone takes .* of max_positions 512"):
            sess.submit_edit(xl_, xll_, yl_, mi([(100, 120)]), **GREEDY_EDIT)
        with pytest.raises(AssertionError, match="silence_tokens"):
            sess.submit(x, xl, y, silence_tokens=(1, 2))
        with pytest.raises(AssertionError, match="silence_tokens"):
            sess.submit_edit(x, xl, y, mi(spec["spans"]), silence_tokens=(1, 2))
        with pytest.raises(AssertionError, match="temperature"):
            sess.submit(x, xl, y, temperature=0.0)
        assert sess.stats()["admitted"] == 0
        t = sess.submit_edit(x, xl, y, mi(spec["spans"]), **GREEDY_EDIT)
        done = {tk: res for tk, res, gen in sess.drain()}
        assert np.array_equal(done[t].cpu().numpy(), g2)
    # the same refusals through `inference` itself, message for message
    for m, exc, msg in bad:
        with pytest.raises(exc, match=msg):
            eng.inference(x.cuda(), xl.cuda(), y.cuda(), m, **GREEDY_EDIT)
    assert np.array_equal(eng.inference(x.cuda(), xl.cuda(), y.cuda(), mi(spec["spans"]), **GREEDY_EDIT).cpu().numpy(), g2)


def test_a_failing_edit_costs_nobody_else_their_results():
    """max_positions sized so that one edit's rearranged prompt fits but its spans cannot end: it comes back as VC_ECAP for its own
    ticket.  An edit whose y holds an out-of-range token id is reported for its own ticket too.  The TTS request and the healthy edit
    decoded next to them equal their oracle runs."""
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from voicecraft_amd import synth
    from voicecraft_amd._lib import EngineError
    _, args, sd, _, _, _ = build_case("tts_greedy")
    K = args.n_codebooks
    xb, xlb, yb = synth.random_prompt(args, 12, 64, seed=1601)
    big = edit_req(xb, xlb, yb, [(10, 18), (40, 47)], **GREEDY_EDIT)
    xo, xlo, yo = synth.random_prompt(args, 5, 30, seed=1602)
    ok_edit = edit_req(xo, xlo, yo, [(8, 14)], **GREEDY_EDIT)
    xt, xlt, yt = synth.random_prompt(args, 4, 12, seed=1603)
    ok_tts = tts_req(xt, xlt, yt, **GREEDY_TTS)
    bad_y = yo.clone()
    bad_y[0, 3, 2] = 5000
    bad_tok = edit_req(xo, xlo, bad_y, [(8, 14)], **GREEDY_EDIT)
    torch.set_num_threads(min(4, torch.get_num_threads()))
    orc = VoiceCraftOracle(args, sd)
    tr = []
    oracle_run(orc, big, trace=tr)
    M = len(big["spans"])
    n_cols = 64 - 15 + (M + 1) * (K + 1) + 1 + 1             # kept frames, K + 1 columns per piece (shift + placeholder), eos, first empty column
    rows_needed = 12 + n_cols + len(tr) + 3 * (M - 1)        # every sampled step but the last adds a position, a switch three
    P = 12 + n_cols + 3 * M + M * (K + 1) + 4                # the prompt passes edit_prepare's room check with a little to spare ...
    assert P < rows_needed - K, (P, rows_needed)             # ... and the spans cannot end inside it
    wants = [oracle_run(orc, ok_tts), oracle_run(orc, ok_edit)]
    # positions the healthy ones use: text + prompt columns + one per sampled step (generated frames + K per span)
    need_tts = 4 + (12 + 1) + (wants[0].shape[2] - 12) + K
    need_edit = 5 + (24 + 2 * (K + 1) + 2) + (wants[1].shape[2] - 24) + K
    assert max(need_tts, need_edit) + 4 <= P, (need_tts, need_edit, P)
    eng = engine_for(args, sd, max_positions=P)
    with pytest.raises(EngineError, match="max_positions"):
        eng.inference_multi([xb[0]], [yb[0]], [big["spans"]], **GREEDY_EDIT)       # the blocking call's outcome for that request
    reqs = [ok_tts, big, bad_tok, ok_edit]
    with eng.open_session(3, top_k=40) as sess:
        tickets = [submit(sess, r) for r in reqs]
        got, failed = _drain_collecting_failures(sess)
        assert sorted(failed) == sorted([tickets[1], tickets[2]]), failed
        assert isinstance(failed[tickets[1]], EngineError) and "max_positions" in str(failed[tickets[1]])
        assert isinstance(failed[tickets[2]], AssertionError) and f"ticket {tickets[2]}" in str(failed[tickets[2]])
        assert "out of range" in str(failed[tickets[2]])
        done = {t: res.cpu().numpy() for t, res, gen in got}
        assert sorted(done) == sorted([tickets[0], tickets[3]])
        assert done[tickets[0]].shape == wants[0].shape and np.array_equal(done[tickets[0]], wants[0])
        assert done[tickets[3]].shape == wants[1].shape and np.array_equal(done[tickets[3]], wants[1])
        # every slot is free again
        again = [submit(sess, r) for r in (ok_edit, ok_tts, ok_edit)]
        more = {t: res.cpu().numpy() for t, res, gen in sess.drain()}
        assert np.array_equal(more[again[0]], wants[1]) and np.array_equal(more[again[1]], wants[0]) and np.array_equal(more[again[2]], wants[1])


def test_inference_queue_equals_inference_multi():
    """7 edits through 3 slots: request by request what inference_multi gives for them (fp32, greedy), in input order."""
    from voicecraft_amd import synth
    _, args, sd, _, _, _ = build_case("tts_greedy")
    xs, ys, ms = [], [], []
    for u, (Lx, T, spans) in enumerate([(9, 64, [(10, 18), (40, 47)]), (6, 40, [(12, 19)]), (8, 45, [(3, 4), (15, 22), (30, 31)]),
                                        (5, 30, [(8, 14)]), (10, 70, [(5, 9), (30, 38)]), (7, 44, [(20, 20)]), (8, 60, [(20, 31)])]):
        x, _, y = synth.random_prompt(args, Lx, T, seed=1700 + u)
        xs.append(x[0]); ys.append(y[0]); ms.append(spans)
    eng = engine_for(args, sd, max_seqs=8)
    want = [w.cpu().numpy() for w in eng.inference_multi(xs, ys, ms, **GREEDY_EDIT)]
    got = eng.inference_queue(xs, ys, ms, max_live=3, **GREEDY_EDIT)
    st = eng.last_session_stats
    assert len(got) == 7 and st["admitted"] == 7 and st["admitted_while_live"] >= 1, st
    for u, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy()
        assert g.shape == w.shape and np.array_equal(g, w), u
