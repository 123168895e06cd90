"""-m gpu: frames of live session tickets (include/vc_engine.h vc_session_frames; DecodeSession.submit(stream=True) / poll_frames).
Every streaming request hands out its frames while the batch it shares goes on decoding: contiguous chunks from frame 0, each of at
least chunk_frames frames except the last, whose concatenation is the `gen` of the request's result - which is the request's own
one-shot call.  What is handed out when hangs on the submission schedule alone, never on how far the device runs ahead."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from test_gpu_session import _engine, _oracle, _workload

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -2


def _stream_run(eng, prompts, max_live, chunk, G, seeds=None, sleeps=(), stream=None, **sampling):
    """The schedule of test_gpu_session._scheduled_run (submit 2, three turns, submit 5, two turns, submit the rest, drain), every
    turn followed by one poll_frames.  Returns the tickets in submission order, per ticket its chunks
    [(first, codes as numpy, done, session idle?, requests admitted so far, turns since its submit)], per ticket (res, gen), stats."""
    eng.set_option("graph_steps", G)
    tickets, chunks, results, born = [], {}, {}, {}
    turns = [0]
    with eng.open_session(max_live, **sampling) as sess:
        def submit(lo, hi):
            for u in range(lo, hi):
                xx, xl, yy = prompts[u]
                t = sess.submit(xx, xl, yy, seed=None if seeds is None else seeds[u], stream=True if stream is None else stream[u])
                tickets.append(t)
                chunks[t] = []
                born[t] = turns[0]

        def turn():
            if sleeps:
                time.sleep(sleeps[turns[0] % len(sleeps)])
            for t, res, gen in sess.poll():
                results[t] = (res.cpu().numpy(), gen.cpu().numpy())
            turns[0] += 1
            admitted = sess.stats()["admitted"]
            for t, first, codes, done in sess.poll_frames(chunk):
                assert codes.shape[0] == 1 and codes.shape[1] == eng.args.n_codebooks, codes.shape
                chunks[t].append((first, codes[0].cpu().numpy(), done, sess.idle, admitted, turns[0] - born[t]))
        submit(0, 2)
        for _ in range(3):
            turn()
        submit(2, 7)
        for _ in range(2):
            turn()
        submit(7, len(prompts))
        while not sess.idle:
            turn()
        turn()                                     # what the last turn's finished tickets still had
        assert sess.poll_frames(chunk) == []
        stats = sess.stats()
    return tickets, chunks, results, stats


def _check_chunks(tickets, chunks, results, chunk, G, K, streamed=None):
    """Contiguous from 0; every chunk but the last at least `chunk` long; done on the last alone; never more than the schedule allows;
    the concatenation is gen."""
    for u, t in enumerate(tickets):
        if streamed is not None and not streamed[u]:
            assert chunks[t] == [], (u, "a ticket that does not stream got frames")
            continue
        cs = chunks[t]
        gen = results[t][1]
        assert cs and cs[-1][2] and not any(c[2] for c in cs[:-1]), (u, [(c[0], c[1].shape[1], c[2]) for c in cs])
        at = 0
        for i, (first, codes, done, _, _, age) in enumerate(cs):
            n = codes.shape[1]
            assert first == at, (u, i, first, at)
            assert n >= chunk or i == len(cs) - 1, (u, i, n, chunk)
            assert first + n <= 1 + G * age - (K - 1), (u, i, first, n, G, age)
            at += n
        got = np.concatenate([c[1] for c in cs], axis=1)
        assert got.shape == gen.shape[1:] and np.array_equal(got, gen[0]), (u, got.shape, gen.shape)


@pytest.mark.parametrize("preset,K,n,max_seqs,max_live,graph", [
    ("tiny", 4, 14, 4, 4, True),
    ("tiny", 4, 14, 4, 3, False),          # a width with a filler row
    ("tiny", 8, 14, 4, 4, True),           # the deepest un-shift
    ("tiny_h16", 4, 40, 20, 20, True),     # 17..64-row steps, re-packs while streaming
])
def test_streamed_frames_are_gen_which_is_the_oracles_run_of_the_utterance_alone(preset, K, n, max_seqs, max_live, graph):
    a, sd, prompts = _workload(preset, n, K)
    want = _oracle(preset, n, K)
    eng = _engine(a, sd, "fp32", max_seqs, graph)
    chunk, G = 8, 4
    tickets, chunks, results, stats = _stream_run(eng, prompts, max_live, chunk, G, top_k=1, stop_repetition=3)
    assert stats["admitted"] == n, stats
    _check_chunks(tickets, chunks, results, chunk, G, K)
    for u, t in enumerate(tickets):
        res = results[t][0]
        assert res.shape == want[u].shape and np.array_equal(res, want[u]), (u, res.shape, want[u].shape)
    # some ticket receives a chunk before it has ended, while the session is decoding and before every request has been admitted
    early = [c for t in tickets for c in chunks[t] if not c[2] and not c[3] and c[4] < n and c[1].shape[1] > 0]
    assert early, "no frame left the session before its request ended"


@pytest.mark.parametrize("G", [1, 8])
@pytest.mark.parametrize("chunk", [1, 8, 25])
def test_chunk_frames_and_graph_steps(chunk, G):
    n, K = 14, 4
    a, sd, prompts = _workload("tiny", n, K)
    want = _oracle("tiny", n, K)
    eng = _engine(a, sd, "fp32", 4)
    tickets, chunks, results, _ = _stream_run(eng, prompts, 4, chunk, G, top_k=1, stop_repetition=3)
    _check_chunks(tickets, chunks, results, chunk, G, K)
    for u, t in enumerate(tickets):
        assert np.array_equal(results[t][0], want[u]), u


def test_what_is_handed_out_when_is_the_same_in_every_run():
    """bf16, top-k 40, seeded: one schedule three times with different sleeps between the calls - the same (first, n) sequence for
    every ticket and the same tokens."""
    n = 14
    a, sd, prompts = _workload("tiny128", n)
    eng = _engine(a, sd, "bf16", 8)
    seeds = [100 + u for u in range(n)]
    runs = []
    for sleeps in ((), (0.0, 0.02, 0.005), (0.03, 0.0)):
        tickets, chunks, results, stats = _stream_run(eng, prompts, 6, 8, 3, seeds=seeds, sleeps=sleeps, top_k=40, stop_repetition=3)
        _check_chunks(tickets, chunks, results, 8, 3, a.n_codebooks)
        runs.append(([[(c[0], c[1].shape[1], c[2]) for c in chunks[t]] for t in tickets], [results[t][0] for t in tickets], stats))
    assert len({r.shape[2] for r in runs[0][1]}) > 1
    for i in (1, 2):
        assert runs[i][0] == runs[0][0], i
        assert runs[i][2] == runs[0][2], (i, runs[i][2], runs[0][2])
        for u in range(n):
            assert runs[i][1][u].shape == runs[0][1][u].shape and np.array_equal(runs[i][1][u], runs[0][1][u]), (i, u)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_one_slot_reused(dtype):
    """max_live = 1: three seeded requests through the same slot.  Each one's streamed frames are inference_tts(_seed=...)'s gen, the
    second and third start at frame 0 (nothing of the slot's previous occupant), and the last chunk ends exactly at Tg although the
    request ended inside a batch."""
    a, sd, prompts = _workload("tiny", 3)
    eng = _engine(a, sd, dtype, 1)
    seeds = [5, 6, 7]
    want = [eng.inference_tts(xx.cuda(), xl.cuda(), yy.cuda(), top_k=40, stop_repetition=3, _seed=s)[1].cpu().numpy()
            for (xx, xl, yy), s in zip(prompts, seeds)]
    G = 8
    assert any((w.shape[2] + a.n_codebooks - 1) % G for w in want), [w.shape for w in want]     # some request ends inside a batch
    eng.set_option("graph_steps", G)
    got = {}
    with eng.open_session(1, top_k=40, stop_repetition=3) as sess:
        tickets = [sess.submit(*p, seed=s, stream=True) for p, s in zip(prompts, seeds)]
        while not sess.idle:
            sess.poll()                                # (the turn that finds the last request finished is the one that finds the session idle)
            for t, first, codes, done in sess.poll_frames(4):
                got.setdefault(t, []).append((first, codes[0].cpu().numpy(), done))
    for u, t in enumerate(tickets):
        assert got[t][0][0] == 0 and got[t][-1][2], (u, got[t][0][0])
        assert [c[0] for c in got[t]] == list(np.cumsum([0] + [c[1].shape[1] for c in got[t]][:-1])), u
        cat = np.concatenate([c[1] for c in got[t]], axis=1)
        assert cat.shape[1] == want[u].shape[2] and np.array_equal(cat, want[u][0]), (u, cat.shape, want[u].shape)


def test_edits_and_streaming_tts_share_a_session():
    """Two editing requests and three streaming TTS requests: the TTS frames are their gen, and the edits equal their result from a
    session in which nobody streams."""
    from test_gpu_session_edit import GREEDY_EDIT, GREEDY_TTS, engine_for
    from _util import build_case
    from voicecraft_amd import synth
    _, args, sd, _, _, _ = build_case("tts_greedy")
    shapes = [("tts", 6, 21, None), ("edit", 9, 64, [(10, 18), (40, 47)]), ("tts", 3, 12, None), ("edit", 8, 60, [(20, 31)]),
              ("tts", 7, 40, None)]
    reqs = [(kind, synth.random_prompt(args, Lx, T, seed=1200 + u), spans) for u, (kind, Lx, T, spans) in enumerate(shapes)]
    eng = engine_for(args, sd)
    eng.set_option("graph_steps", 2)

    def run(stream):
        frames, done = {}, {}
        with eng.open_session(3, top_k=40, stop_repetition=3) as sess:
            tickets = []
            for kind, (x, xl, y), spans in reqs:
                if kind == "tts":
                    tickets.append(sess.submit(x, xl, y, stream=stream, **GREEDY_TTS))
                else:
                    tickets.append(sess.submit_edit(x, xl, y, torch.tensor([spans], dtype=torch.int64), **GREEDY_EDIT))
            while not sess.idle:
                for t, res, gen in sess.poll():
                    done[t] = (res.cpu().numpy(), None if gen is None else gen.cpu().numpy())
                for t, first, codes, d in sess.poll_frames(4):
                    frames.setdefault(t, []).append((first, codes[0].cpu().numpy(), d))
        return tickets, frames, done
    t0, f0, d0 = run(False)
    assert f0 == {}
    t1, f1, d1 = run(True)
    for u, (kind, _, _) in enumerate(reqs):
        assert np.array_equal(d0[t0[u]][0], d1[t1[u]][0]), (u, kind)
        if kind == "edit":
            assert t1[u] not in f1
        else:
            cs = f1[t1[u]]
            assert cs[0][0] == 0 and cs[-1][2]
            assert np.array_equal(np.concatenate([c[1] for c in cs], axis=1), d1[t1[u]][1][0]), u


def _frames(eng, tickets, min_frames, cap):
    K, n = eng.args.n_codebooks, len(tickets)
    buf = torch.full((max(n, 1), K, max(cap, 1)), -7, dtype=torch.int64, device=eng.device)
    first, cnt, done = (C.c_int * max(n, 1))(), (C.c_int * max(n, 1))(), (C.c_int * max(n, 1))()
    torch.cuda.synchronize()
    rc = eng.lib.vc_session_frames(eng._h, n, (C.c_int * max(n, 1))(*tickets), min_frames, C.c_void_p(buf.data_ptr()), cap, first, cnt, done)
    return rc, list(first)[:n], list(cnt)[:n], list(done)[:n], buf.cpu().numpy(), eng.lib.vc_last_error(eng._h).decode()


def test_refusals_leave_every_cursor_where_it_was():
    from test_gpu_session_edit import GREEDY_EDIT
    from _util import build_case
    from voicecraft_amd import synth
    _, args, sd, _, _, _ = build_case("tts_greedy")
    from test_gpu_session_edit import engine_for
    eng = engine_for(args, sd)
    rc, *_ = _frames(eng, [1], 1, 8)
    assert rc == ESTATE                                                    # no session
    G, K = 4, args.n_codebooks
    eng.set_option("graph_steps", G)
    p = [synth.random_prompt(args, 5, 20 + u, seed=40 + u) for u in range(6)]
    with eng.open_session(3, top_k=1, stop_repetition=3) as sess:
        ta, tb = sess.submit(*p[0]), sess.submit(*p[1])
        te = sess.submit_edit(*p[2], torch.tensor([[(5, 9)]], dtype=torch.int64), **GREEDY_EDIT)
        tp = sess.submit(*p[3])                                            # no slot for it: pending
        rc, first, cnt, done, _, _ = _frames(eng, [ta, tb, tp], 1, 64)
        assert rc == 0 and cnt == [0, 0, 0] and done == [0, 0, 0]          # nothing is admitted before the first turn
        res = {}
        for _ in range(4):
            res.update({t: (r, g) for t, r, g in sess.poll()})
        assert ta not in res and tb not in res
        # two batches have been seen to end: 1 + 2 G rows each, whatever the device has done since
        rc, first, cnt, done, buf, _ = _frames(eng, [ta], 1, 3)
        assert rc == 0 and first == [0] and cnt == [3] and done == [0], (rc, first, cnt, done)
        avail = 1 + 2 * G - (K - 1)
        for bad, msg in (([te], "editing requests do not stream"), ([ta, te], "editing requests do not stream"), ([ta, 999], "unknown ticket"),
                         ([ta, tb, ta], "twice"), ([ta, tb, tp, tb], "max_live")):
            rc, _, _, _, _, err = _frames(eng, bad, 1, 64)
            assert rc == EINVAL and msg in err, (bad, rc, err)
        for mf, cap in ((9, 8), (0, 8), (1, 0)):
            rc, _, _, _, _, err = _frames(eng, [ta, tb], mf, cap)
            assert rc == EINVAL and "min_frames" in err, (mf, cap, rc, err)
        assert _frames(eng, [], 1, 8)[0] == EINVAL
        assert eng.lib.vc_session_frames(eng._h, 1, None, 1, None, 8, None, None, None) == EINVAL
        # the pending ticket: known, 0 frames, not done; the cursors of the others are where the one good call left them
        rc, first, cnt, done, buf, _ = _frames(eng, [tp, ta, tb], 1, 64)
        assert rc == 0 and first == [0, 3, 0] and cnt == [0, avail - 3, avail] and done == [0, 0, 0], (first, cnt, done)
        assert (buf[0] == -7).all() and (buf[1, :, avail - 3:] == -7).all() and (buf[2, :, avail:] == -7).all()
        head_b = buf[2, :, :avail].copy()
        # fewer ready than min_frames: nothing, and nothing moves
        rc, first, cnt, done, _, _ = _frames(eng, [ta, tb], 60, 64)
        assert rc == 0 and first == [avail, avail] and cnt == [0, 0], (first, cnt)
        res.update({t: (r, g) for t, r, g in sess.drain()})
        assert sorted(res) == sorted([ta, tb, te, tp])
        rc, _, _, _, _, err = _frames(eng, [tb], 1, 64)
        assert rc == EINVAL and "unknown ticket" in err                    # fetched
        gen_b = res[tb][1].cpu().numpy()[0]
        assert gen_b.shape[1] >= avail + K, "the recipe's request ended inside the first two batches: choose another prompt"
        assert np.array_equal(head_b - (int(args.n_special) if args.special_first else 0), gen_b[:, :avail])


def test_a_finished_ticket_streams_until_it_is_fetched_even_when_its_retirement_was_not_reported():
    """vc_session_advance with no room in tickets_out leaves a retired request live on the host: the frames stop at its own end all
    the same (counted from its record), and go on being handed out until the fetch."""
    n, K, G = 2, 4, 8
    a, sd, prompts = _workload("tiny", n, K)
    want = _oracle("tiny", 14, K)[:n]                                     # (the ragged recipe's first two; its oracle runs are shared)
    eng = _engine(a, sd, "fp32", 2)
    eng.set_option("graph_steps", G)
    with eng.open_session(2, top_k=1, stop_repetition=3) as sess:
        tk = [sess.submit(*prompts[u]) for u in range(n)]
        nfin, idle = C.c_int(0), C.c_int(0)
        for _ in range(40):                                               # cap = 0: nothing can be reported
            assert eng.lib.vc_session_advance(eng._h, None, 0, C.byref(nfin), C.byref(idle)) == 0 and nfin.value == 0
        for u in range(n):
            T = prompts[u][2].shape[1]
            gen = want[u][0][:, T:]
            rc, first, cnt, done, buf, _ = _frames(eng, [tk[u]], 1, 256)
            assert rc == 0 and first == [0] and cnt == [gen.shape[1]] and done == [1], (u, first, cnt, done, gen.shape)
            shift = int(a.n_special) if a.special_first else 0
            assert np.array_equal(buf[0, :, : cnt[0]] - shift, gen), u
            assert _frames(eng, [tk[u]], 1, 256)[1:4] == ([gen.shape[1]], [0], [1])
        got = {t: r.cpu().numpy() for t, r, g in sess.drain()}
        for u in range(n):
            assert np.array_equal(got[tk[u]], want[u]), u


def test_a_request_without_a_result_is_done_and_the_others_stream_to_their_end():
    """The request that runs out of max_positions (test_gpu_session's recipe): done, and fetch raises VC_ECAP; a prompt that alone
    does not fit is refused at submit and streams nothing; a request with an out-of-range token id never hands out a frame."""
    from voicecraft_amd import synth
    from voicecraft_amd._lib import EngineError
    from voicecraft_amd.engine import SessionRequestError, VoiceCraftEngine
    n = 14
    a, sd, prompts = _workload("tiny", n)
    want = _oracle("tiny", n)
    K = a.n_codebooks
    need = [int(p[1][0]) + w.shape[2] + 1 + K for p, w in zip(prompts, want)]
    big = max(range(n), key=lambda u: need[u])
    P = need[big] - 6
    healthy = [u for u in range(n) if need[u] <= P - 6][:4]
    assert len(healthy) >= 4 and P >= 40, (need, P)
    eng = VoiceCraftEngine(a, sd, device="cuda:0", dtype="fp32", max_seqs=4, max_positions=P)
    eng.set_option("graph_steps", 4)
    bad_y = prompts[healthy[0]][2].clone()
    bad_y[0, 3, 2] = 5000
    frames, done, failed = {}, {}, {}
    with eng.open_session(3, top_k=1, stop_repetition=3) as sess:
        with pytest.raises(EngineError, match="max_positions"):
            sess.submit(*synth.random_prompt(a, 8, 520, seed=3), stream=True)
        tickets = {u: sess.submit(*prompts[u], stream=True) for u in healthy[:2] + [big] + healthy[2:]}
        t_bad = sess.submit(prompts[healthy[0]][0], prompts[healthy[0]][1], bad_y, stream=True)
        for _ in range(400):
            if sess.idle:
                break
            try:
                for t, res, gen in sess.poll():
                    done[t] = gen.cpu().numpy()
            except SessionRequestError as ex:
                failed.update(ex.failed)
            for t, first, codes, d in sess.poll_frames(4):
                frames.setdefault(t, []).append((first, codes[0].cpu().numpy(), d))
        assert sess.idle
        for t, res, gen in sess.poll():
            done[t] = gen.cpu().numpy()
    assert sorted(failed) == sorted([tickets[big], t_bad]), failed
    assert isinstance(failed[tickets[big]], EngineError) and "code -4" in str(failed[tickets[big]]) and "max_positions" in str(failed[tickets[big]])
    assert frames[tickets[big]][-1][2]                                      # done, though there is no result
    assert frames[t_bad][-1][2] and sum(c[1].shape[1] for c in frames[t_bad]) == 0
    for u in healthy:
        cs = frames[tickets[u]]
        T = prompts[u][2].shape[1]
        assert cs[-1][2] and np.array_equal(np.concatenate([c[1] for c in cs], axis=1), want[u][0][:, T:]), u
        assert np.array_equal(done[tickets[u]][0], want[u][0][:, T:]), u
