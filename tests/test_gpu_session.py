"""-m gpu: decode sessions (continuous batching, include/vc_engine.h vc_session_*).  Requests join a running batch between two graph
batches and leave it as soon as they end; every request must still be its own `inference_tts` call: in exact mode equal to the
oracle's run of that utterance alone, whatever it shared a step with, and with sampling bit-equal to the one-shot call with its seed."""
import time

import numpy as np
import pytest
import torch

from test_gpu_model import engine_run, make_engine
from _util import load_golden

pytestmark = pytest.mark.gpu

_ORACLE = {}      # (preset, K) -> the oracle's greedy results of the ragged recipe's first utterances, computed once


def _workload(preset, n, K=4):
    """The ragged recipe of tests/test_gpu_options.py: live terminators, 14 different prompt shapes."""
    from voicecraft_amd import synth
    a = synth.make_args(preset, n_codebooks=K)
    sd = synth.make_state_dict(a, seed=4, mute_eos=False, boost=[(0, 2051, 0.45)])
    prompts = [synth.random_prompt(a, 4 + (u % 5), 9 + 3 * (u % 7), seed=700 + u) for u in range(n)]
    return a, sd, prompts


def _oracle(preset, n, K=4):
    from oracle.voicecraft_oracle import VoiceCraftOracle
    have = _ORACLE.get((preset, K), [])
    if len(have) < n:
        a, sd, prompts = _workload(preset, n, K)
        torch.set_num_threads(min(4, torch.get_num_threads()))
        orc = VoiceCraftOracle(a, sd)
        have = have + [orc.inference_tts(xx, xl, yy, top_k=1, stop_repetition=3)[0].numpy() for (xx, xl, yy) in prompts[len(have):]]
        _ORACLE[(preset, K)] = have
    want = have[:n]
    _, _, prompts = _workload(preset, n, K)
    lens = [w.shape[2] - p[2].shape[1] for w, p in zip(want, prompts)]
    assert min(lens) * 2 <= max(lens), lens                       # the workload really is ragged
    return want


def _engine(a, sd, dtype, max_seqs, graph=True):
    from voicecraft_amd.engine import VoiceCraftEngine
    return VoiceCraftEngine(a, sd, device="cuda:0", dtype=dtype, max_seqs=max_seqs, max_positions=256, use_graph=graph)


def _assert_equal(got, want, tag=None):
    assert len(got) == len(want), (len(got), len(want))
    for u, ((res, gen), w) in enumerate(zip(got, want)):
        r = res.cpu().numpy()
        assert r.shape == w.shape and np.array_equal(r, w), (tag, u, r.shape, w.shape)


@pytest.mark.parametrize("preset,K,n,max_seqs,max_live,graph", [
    ("tiny", 4, 14, 4, 4, True),
    ("tiny", 4, 14, 4, 3, False),          # a width with a filler row
    ("tiny128", 4, 14, 8, 6, True),
    ("tiny_h16", 4, 40, 20, 20, True),     # the 17..64-row wide step with admissions
    ("tiny", 8, 10, 4, 4, True),
])
def test_greedy_fp32_every_request_equals_its_own_oracle_run(preset, K, n, max_seqs, max_live, graph):
    a, sd, prompts = _workload(preset, n, K)
    want = _oracle(preset, n, K)
    eng = _engine(a, sd, "fp32", max_seqs, graph)
    got = eng.inference_tts_queue([p[0][0] for p in prompts], [p[2][0] for p in prompts], max_live=max_live, top_k=1, stop_repetition=3)
    st = eng.last_session_stats
    print(st)
    _assert_equal(got, want, st)
    assert st["admitted"] == n and st["admitted_while_live"] >= 1, st
    assert 0 < st["live_rows"] <= st["launched_rows"], st
    if preset == "tiny_h16":
        assert st["widenings"] + st["narrowings"] >= 1, st


def _scheduled_run(eng, prompts, max_live, seeds=None, **sampling):
    """Submit 2 requests, poll three turns, submit 5 more, poll twice, submit the rest, drain."""
    events, tickets = [], []
    with eng.open_session(max_live, **sampling) as sess:
        def submit(lo, hi):
            for u in range(lo, hi):
                xx, xl, yy = prompts[u]
                tickets.append(sess.submit(xx, xl, yy, seed=None if seeds is None else seeds[u]))

        def poll():
            for t, res, gen in sess.poll():
                events.append((t, res, gen, sess.idle, sess.stats()["admitted"]))
        submit(0, 2)
        for _ in range(3):
            poll()
        submit(2, 7)
        for _ in range(2):
            poll()
        submit(7, len(prompts))
        while not sess.idle:
            poll()
        stats = sess.stats()
    done = {t: (res, gen) for t, res, gen, _, _ in events}
    return [done[t] for t in tickets], events, stats


def test_submitting_while_decoding():
    n = 14
    a, sd, prompts = _workload("tiny", n)
    want = _oracle("tiny", n)
    eng = _engine(a, sd, "fp32", 4)
    got, events, stats = _scheduled_run(eng, prompts, 4, top_k=1, stop_repetition=3)
    _assert_equal(got, want, stats)
    assert len(events) == n and stats["admitted"] == n and stats["admitted_while_live"] >= 1, stats
    # results are handed out while the session is still decoding: the first one before every request has even been admitted
    first = events[0]
    assert not first[3] and first[4] < n, (first[3], first[4])
    assert sum(1 for ev in events if not ev[3]) >= n - 4, [ev[3] for ev in events]


def test_idle_and_restart():
    n = 9
    a, sd, prompts = _workload("tiny", n)
    want = _oracle("tiny", n)
    eng = _engine(a, sd, "fp32", 4)
    with eng.open_session(4, top_k=1, stop_repetition=3) as sess:
        t0 = [sess.submit(*prompts[u]) for u in range(5)]
        done = {t: (res, gen) for t, res, gen in sess.drain()}
        assert sess.idle and sorted(done) == sorted(t0)
        turns = sess.stats()["turns"]
        assert sess.poll() == [] and sess.idle                       # an idle session queues nothing
        assert sess.stats()["turns"] == turns + 1
        rows_idle = sess.stats()["launched_rows"]
        assert sess.poll() == [] and sess.stats()["launched_rows"] == rows_idle
        t1 = [sess.submit(*prompts[u]) for u in range(5, n)]
        done.update({t: (res, gen) for t, res, gen in sess.drain()})
        assert sess.idle and sess.stats()["admitted"] == n
    _assert_equal([done[t] for t in t0 + t1], want)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_one_slot_reused_is_bit_equal_to_the_one_shot_call(dtype):
    """max_live = 1: three sampled requests run one after the other through the same slot; each equals inference_tts with its seed on
    the same engine (the same width-1 kernels): the per-request Philox key, the reset of the state, the overwrite of the K/V slot."""
    a, sd, prompts = _workload("tiny", 3)
    eng = _engine(a, sd, dtype, 1)
    seeds = [5, 6, 7]
    want = [eng.inference_tts(xx.cuda(), xl.cuda(), yy.cuda(), top_k=40, stop_repetition=3, _seed=s)[0].cpu().numpy()
            for (xx, xl, yy), s in zip(prompts, seeds)]
    assert len({w.shape[2] for w in want}) > 1 or not np.array_equal(want[0], want[1])
    got = eng.inference_tts_queue([p[0][0] for p in prompts], [p[2][0] for p in prompts], max_live=1, seeds=seeds, top_k=40,
                                  stop_repetition=3)
    _assert_equal(got, want, dtype)
    st = eng.last_session_stats
    assert st["admitted"] == 3 and st["admitted_while_live"] == 0 and st["widenings"] == st["narrowings"] == 0, st
    # and the one-shot call is untouched by the session before it
    again = eng.inference_tts(prompts[0][0].cuda(), prompts[0][1].cuda(), prompts[0][2].cuda(), top_k=40, stop_repetition=3, _seed=5)[0]
    assert np.array_equal(again.cpu().numpy(), want[0])


def test_sampled_bf16_tokens_and_stats_are_the_same_in_every_run():
    """bf16, top-k sampling, live terminators: the width a step runs at decides which kernels round its logits, so who is admitted when
    must not depend on how far the device has run ahead of the host.  Six runs of one submission schedule, the host disturbed
    differently before each: the same tokens and the same counters."""
    n = 14
    a, sd, prompts = _workload("tiny128", n)
    eng = _engine(a, sd, "bf16", 8)
    eng.set_option("graph_steps", 3)
    seeds = [100 + u for u in range(n)]
    runs, stats = [], []
    for i in range(6):
        if i % 2:
            time.sleep(0.02 * i)                      # another phase between the host's loop and the device's
        got, _, st = _scheduled_run(eng, prompts, 6, seeds=seeds, top_k=40, stop_repetition=3)
        runs.append([res.cpu().numpy() for res, gen in got])
        stats.append(st)
    lens = [r.shape[2] for r in runs[0]]
    assert len(set(lens)) > 1, lens
    assert stats[0]["admitted_while_live"] >= 1 and stats[0]["widenings"] + stats[0]["narrowings"] >= 1, stats[0]
    for i in range(1, 6):
        assert stats[i] == stats[0], (i, stats[i], stats[0])
        for u in range(n):
            assert runs[i][u].shape == runs[0][u].shape and np.array_equal(runs[i][u], runs[0][u]), (i, u)


def test_refusals_and_recovery():
    from voicecraft_amd import synth
    from voicecraft_amd._lib import EngineError
    eng, spec, x, x_lens, y = make_engine("tts_greedy", "fp32")
    a = eng.args
    multi_in = ([x[0, : int(x_lens[0])].cpu()] * 2, [y[0].cpu()] * 2)
    before = [r.cpu().numpy() for r, g in eng.inference_tts_multi(*multi_in, top_k=1, stop_repetition=3)]
    with pytest.raises(AssertionError, match="not supported"):
        eng.open_session(2, batch_size=3)
    sess = eng.open_session(2, top_k=1, stop_repetition=3)
    for call in (lambda: eng.inference_tts(x, x_lens, y, top_k=1),
                 lambda: eng.inference_tts_multi(*multi_in, top_k=1),
                 lambda: eng.inference(x, x_lens, y, torch.tensor([[[2, 4]]]), top_k=1),
                 lambda: eng.set_option("shrink", 0),
                 lambda: next(eng.inference_tts_stream(x, x_lens, y, top_k=1)),
                 lambda: eng.open_session(2)):
        with pytest.raises(EngineError, match="session"):
            call()
    # a prompt that alone does not fit max_positions (512 here) is refused at submit, and the session goes on
    xl, xll, yl = synth.random_prompt(a, 8, 520, seed=3)
    with pytest.raises(EngineError, match="max_positions"):
        sess.submit(xl, xll, yl)
    with pytest.raises(AssertionError, match="unknown ticket"):
        sess.fetch(12345)
    t0 = sess.submit(x, x_lens, y)
    with pytest.raises(EngineError, match="not finished"):
        sess.fetch(t0)
    done = {t: res for t, res, gen in sess.drain()}
    assert np.array_equal(done[t0].cpu().numpy(), load_golden("tts_greedy")["res"])
    with pytest.raises(AssertionError, match="unknown ticket"):
        sess.fetch(t0)                                                # fetched already
    # close with requests live and pending: the engine is reusable
    for _ in range(5):
        sess.submit(x, x_lens, y)
    sess.poll()
    sess.poll()
    sess.close()
    got, _ = engine_run(eng, spec, x, x_lens, y)
    assert np.array_equal(got.cpu().numpy(), load_golden("tts_greedy")["res"])
    after = [r.cpu().numpy() for r, g in eng.inference_tts_multi(*multi_in, top_k=1, stop_repetition=3)]
    assert all(np.array_equal(b, c) for b, c in zip(before, after))
    with eng.open_session(2, top_k=1, stop_repetition=3) as s2:     # ... and a new session opens
        t1 = s2.submit(x, x_lens, y)
        assert np.array_equal(dict((t, r) for t, r, g in s2.drain())[t1].cpu().numpy(), load_golden("tts_greedy")["res"])


def _drain_collecting_failures(sess):
    from voicecraft_amd.engine import SessionRequestError
    failed = {}
    for _ in range(64):
        try:
            return sess.drain(), failed
        except SessionRequestError as ex:
            failed.update(ex.failed)
    raise AssertionError("the session did not drain")


def test_a_request_that_runs_out_of_positions_does_not_cost_the_others_their_results():
    """One request cannot fit max_positions (vc_tts's VC_ECAP, reported at fetch) next to healthy ones in the same session: the
    healthy ones equal the oracle, the failure names its ticket, its slot is free again and the session goes on."""
    from voicecraft_amd._lib import EngineError
    n = 14
    a, sd, prompts = _workload("tiny", n)
    want = _oracle("tiny", n)
    K = a.n_codebooks
    # cache positions a request ends up using: prompt rows + one per generated step (generated frames + K steps)
    need = [int(p[1][0]) + w.shape[2] + 1 + K for p, w in zip(prompts, want)]
    big = max(range(n), key=lambda u: need[u])
    P = need[big] - 6                                         # the neediest request runs out ...
    healthy = [u for u in range(n) if need[u] <= P - 6][:6]    # ... the ones well below the line do not
    assert len(healthy) >= 4 and P >= 40, (need, P)
    from voicecraft_amd.engine import VoiceCraftEngine
    eng = VoiceCraftEngine(a, sd, device="cuda:0", dtype="fp32", max_seqs=4, max_positions=P)
    with pytest.raises(EngineError, match="max_positions"):   # the one-shot call's outcome for that utterance
        eng.inference_tts(prompts[big][0].cuda(), prompts[big][1].cuda(), prompts[big][2].cuda(), top_k=1, stop_repetition=3)
    order = healthy[:2] + [big] + healthy[2:]
    with eng.open_session(3, top_k=1, stop_repetition=3) as sess:
        tickets = {u: sess.submit(*prompts[u]) for u in order}
        got, failed = _drain_collecting_failures(sess)
        assert sorted(failed) == [tickets[big]], failed
        assert isinstance(failed[tickets[big]], EngineError) and "max_positions" in str(failed[tickets[big]])
        done = {t: res for t, res, gen in got}
        assert sorted(done) == sorted(tickets[u] for u in healthy)
        for u in healthy:
            assert np.array_equal(done[tickets[u]].cpu().numpy(), want[u]), u
        # every slot is free again: three more requests run together
        again = [sess.submit(*prompts[u]) for u in healthy[:3]]
        more = {t: res for t, res, gen in sess.drain()}
        assert sess.stats()["admitted"] == len(order) + 3
        for t, u in zip(again, healthy[:3]):
            assert np.array_equal(more[t].cpu().numpy(), want[u]), u


def test_an_out_of_range_token_id_is_reported_for_its_own_ticket():
    """prompt_k's error bit per request: the request whose y holds an id outside the vocabulary (and the one whose x does) fail at
    fetch, naming their tickets, without a synchronisation per turn; the requests decoded next to them equal the oracle."""
    n = 6
    a, sd, prompts = _workload("tiny", n)
    want = _oracle("tiny", n)
    eng = _engine(a, sd, "fp32", 4)
    bad_y = prompts[1][2].clone()
    bad_y[0, 3, 2] = 5000
    bad_x = prompts[2][0].clone()
    bad_x[0, 1] = 100000
    with eng.open_session(4, top_k=1, stop_repetition=3) as sess:
        t_ok = [sess.submit(*prompts[u]) for u in (0, 3)]
        t_bad = [sess.submit(prompts[1][0], prompts[1][1], bad_y), sess.submit(bad_x, prompts[2][1], prompts[2][2])]
        t_ok += [sess.submit(*prompts[u]) for u in (4, 5)]
        got, failed = _drain_collecting_failures(sess)
        assert sorted(failed) == sorted(t_bad), failed
        for t in t_bad:
            assert isinstance(failed[t], AssertionError) and f"ticket {t}" in str(failed[t]) and "out of range" in str(failed[t])
        done = {t: res for t, res, gen in got}
        assert sorted(done) == sorted(t_ok)
        for t, u in zip(t_ok, (0, 3, 4, 5)):
            assert np.array_equal(done[t].cpu().numpy(), want[u]), u
    # the engine-wide error word was not raised by them: the next blocking call runs
    out = eng.inference_tts(prompts[0][0].cuda(), prompts[0][1].cuda(), prompts[0][2].cuda(), top_k=1, stop_repetition=3)[0]
    assert np.array_equal(out.cpu().numpy(), want[0])
