"""-m gpu: cancelling a request of a decode session (include/vc_engine.h vc_session_cancel; DecodeSession.cancel,
SessionStreamer.cancel).  A pending request leaves the queue, a finished one frees its slot at once, the rows of a live one are retired
by the next turn (session_cancel_k) and its slots come back two turns later, the way any retirement's do.  Whatever is cancelled
when, every other request must still be its own blocking call - bit equality of token ids throughout - and who is admitted when must
stay a function of the schedule of submissions and cancels.

Placing a cancel without looking at the device (graph_steps = 3): a request of n sampled steps admitted by the turn that queues batch a
takes step 0 in that turn and step j >= 1 in batch a + (j - 1) // 3, its last in batch r = a + ceil((n - 1) / 3) - 1.  While a session
has never been idle every turn queues one batch, so the turn made when stats()["turns"] == c queues batch c."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from test_gpu_session import _engine, _oracle, _workload

pytestmark = pytest.mark.gpu

G = 3
GREEDY = dict(top_k=1, stop_repetition=3)


def _steps(want, prompts, K=4):
    """Sampled steps of every utterance's own run: its generated frames + K."""
    return [w.shape[2] - p[2].shape[1] + K for w, p in zip(want, prompts)]


def _last_batch(a, n):
    return a + -(-(n - 1) // G) - 1


def _tiny(n=14, max_seqs=6, graph=True, preset="tiny"):
    a, sd, prompts = _workload(preset, n)
    want = _oracle(preset, n)
    eng = _engine(a, sd, "fp32", max_seqs, graph)
    eng.set_option("graph_steps", G)
    return eng, prompts, want, _steps(want, prompts)


def _same(res, want):
    r = res.cpu().numpy()
    return r.shape == want.shape and np.array_equal(r, want)


def _slots(eng, max_live):
    return eng.debug_read("session_slots", (max_live + 1,), torch.int32).tolist()[1:]


# ------------------------------------------------------------------------------------------------ 1. survivors are untouched
def test_survivors_equal_their_oracle_runs():
    """Six slots, fourteen requests; requests 0, 2, 7 and 12 (35, 36, 37 and 40 steps) are each cancelled before the turn that queues
    batch a + 3, a being the batch of their admission: three batches into their life and at least two before their last."""
    eng, prompts, want, n = _tiny()
    victims = (0, 2, 7, 12)
    with eng.open_session(6, **GREEDY) as sess:
        tickets = [sess.submit(*p) for p in prompts]
        adm, done, cancelled_at = {}, {}, {}
        while not sess.idle:
            c = sess.stats()["turns"]                       # the turn below queues batch c
            for u in victims:
                if u in adm and c == adm[u] + 3:
                    assert _last_batch(adm[u], n[u]) - c >= 2, (u, adm[u], n[u])
                    assert sess.cancel(tickets[u]) == "live"
                    cancelled_at[u] = c
            before = sess.stats()
            for t, res, gen in sess.poll():
                assert t not in done
                done[t] = res
            st = sess.stats()
            assert sess.idle or st["launched_rows"] > before["launched_rows"], (c, st)     # (one batch per turn)
            for u in range(before["admitted"], st["admitted"]):
                adm[u] = c                                  # FIFO, and nothing pending was cancelled: request u is the u-th admitted
        st = sess.stats()
        assert sess.idle and sorted(cancelled_at) == list(victims), (cancelled_at, adm)
        assert st["admitted"] == len(prompts) and sess.cancelled == 4, st
        assert 0 < st["live_rows"] <= st["launched_rows"], st
        assert _slots(eng, 6) == [-1] * 6
    assert sorted(done) == sorted(tickets[u] for u in range(len(prompts)) if u not in victims)
    for u in range(len(prompts)):
        if u not in victims:
            assert _same(done[tickets[u]], want[u]), u


# ------------------------------------------------------------------------------------------------ 2. the slot comes back on schedule
@pytest.mark.parametrize("graph", [True, False])
def test_the_slot_comes_back_clean_two_batches_later(graph):
    """max_live = 2: request 4 (50 steps) and request 5 (20 steps) live, request 3 pending.  Request 4 is cancelled before the turn
    that queues batch 2: the turn that queues batch 4 admits request 3 - not the one before, not the one after; without the cancel
    the first free slot is request 5's, fetched by the turn that queues batch 8."""
    eng, prompts, want, n = _tiny(6, max_seqs=2, graph=graph)
    c = 2
    assert _last_batch(0, n[5]) + 2 > c + 2 and n[4] > n[5]
    with eng.open_session(2, **GREEDY) as sess:
        tl, ts, tp = sess.submit(*prompts[4]), sess.submit(*prompts[5]), sess.submit(*prompts[3])
        done, admitted = {}, []
        for turn in range(c + 4):
            if turn == c:
                assert sess.stats()["turns"] == c
                assert sess.cancel(tl) == "live"
            done.update({t: res for t, res, gen in sess.poll()})
            admitted.append(sess.stats()["admitted"])
        assert admitted == [2] * (c + 2) + [3, 3], admitted
        done.update({t: res for t, res, gen in sess.drain()})
        assert sess.idle and sorted(done) == sorted([ts, tp])
    assert _same(done[ts], want[5]) and _same(done[tp], want[3])


# ------------------------------------------------------------------------------------------------ 3. the race
@pytest.mark.parametrize("late", [0, 1])
def test_a_cancel_that_races_the_requests_own_end(late):
    """Request 5 (20 steps, admitted in front of batch 0) takes its last step in batch r = 6.  late = 0: cancelled before the turn that
    queues batch r + 1 - batch r is in flight, the row has retired by itself and the host cannot know: session_cancel_k must leave
    it alone (its record stands, n_active is lowered once).  late = 1: cancelled before the turn that queues batch r + 2, which finds
    the ticket finished: the cancel wins.  Either way it is never reported, its neighbours are untouched and the session goes idle."""
    eng, prompts, want, n = _tiny(7, max_seqs=3)
    r = _last_batch(0, n[5])
    assert r == 6 and min(n[0], n[1]) > n[5] + 2 * G
    with eng.open_session(3, **GREEDY) as sess:
        t0, t1, tv = sess.submit(*prompts[0]), sess.submit(*prompts[1]), sess.submit(*prompts[5])
        done = {}
        for _ in range(r + 1 + late):
            done.update({t: res for t, res, gen in sess.poll()})
        assert done == {} and sess.stats()["turns"] == r + 1 + late
        assert sess.cancel(tv) == "live"
        for _ in range(64):
            if sess.idle:
                break
            done.update({t: res for t, res, gen in sess.poll()})
        assert sess.idle and sorted(done) == sorted([t0, t1])
        assert _same(done[t0], want[0]) and _same(done[t1], want[1])
        assert _slots(eng, 3) == [-1] * 3
        t6 = sess.submit(*prompts[6])
        more = {t: res for t, res, gen in sess.drain()}
        assert sorted(more) == [t6] and _same(more[t6], want[6])
        assert sess.stats()["admitted"] == 4


# ------------------------------------------------------------------------------------------------ 4. pending, finished, refusals
def test_a_pending_ticket_leaves_the_line():
    eng, prompts, want, n = _tiny(11, max_seqs=2)
    order = [5, 3, 6, 9, 10]
    with eng.open_session(2, **GREEDY) as sess:
        tickets = [sess.submit(*prompts[u]) for u in order]
        done, first_seen = {}, {}
        done.update({t: res for t, res, gen in sess.poll()})
        assert sess.stats()["admitted"] == 2
        assert sess.cancel(tickets[2]) == "pending"
        turn = 1
        while not sess.idle:
            done.update({t: res for t, res, gen in sess.poll()})
            for t in _slots(eng, 2):
                if t >= 0:
                    first_seen.setdefault(t, turn)
            turn += 1
        assert sess.stats()["admitted"] == 4 < len(order) and sess.cancelled == 1
        assert tickets[2] not in first_seen and tickets[2] not in done
        assert first_seen[tickets[3]] <= first_seen[tickets[4]], first_seen       # the ones behind it, in their order
    for i, u in enumerate(order):
        if i != 2:
            assert _same(done[tickets[i]], want[u]), u


def test_a_finished_ticket_frees_its_slot_at_once_and_refusals_name_the_ticket():
    from voicecraft_amd._lib import EngineError
    eng, prompts, want, n = _tiny(7, max_seqs=1)
    lib, h = eng.lib, eng._h
    r = _last_batch(0, n[5])
    with eng.open_session(1, **GREEDY) as sess:
        tv = sess.submit(*prompts[5])
        nf, idle, was = C.c_int(0), C.c_int(0), C.c_int(-1)
        # cap = 0: the turn that queues batch r + 2 has seen batch r end, but has no room to report the ticket - finished, unreported
        for _ in range(r + 3):
            assert lib.vc_session_advance(h, None, 0, C.byref(nf), C.byref(idle)) == 0 and nf.value == 0 and idle.value == 0
        assert _slots(eng, 1) == [tv]
        assert lib.vc_session_cancel(h, tv, C.byref(was)) == 0 and was.value == 2
        assert _slots(eng, 1) == [-1]
        for bad in (tv, 999):
            assert lib.vc_session_cancel(h, bad, None) == -1
            assert f"ticket {bad}".encode() in lib.vc_last_error(h), lib.vc_last_error(h)
            with pytest.raises(EngineError, match=f"unknown ticket {bad}"):
                sess.cancel(bad)
        assert lib.vc_session_fetch(h, tv, None, 0, None, None) == -1 and b"unknown ticket" in lib.vc_last_error(h)
        t6 = sess.submit(*prompts[6])                                  # the session goes on
        got = {t: res for t, res, gen in sess.drain()}
        assert sorted(got) == [t6] and _same(got[t6], want[6])
        st = sess.stats()
        assert st["admitted"] == 2 and st["live_rows"] == (n[5] - 1) + (n[6] - 1), (st, n)
    sess2 = eng.open_session(1, **GREEDY)
    sess2.close()
    with pytest.raises(AssertionError, match="closed"):
        sess2.cancel(1)


# ------------------------------------------------------------------------------------------------ 5. cancel everything
def test_cancelling_everything_leads_to_idle_and_a_submit_restarts():
    """Three live and one pending, all cancelled before the turn that queues batch 3: that turn and the next still queue a batch (the
    host has not seen the retirements), the turn after them finds nothing live and goes idle."""
    eng, prompts, want, n = _tiny(7, max_seqs=3)
    assert min(n[:4]) > 1 + 5 * G
    with eng.open_session(3, **GREEDY) as sess:
        tickets = [sess.submit(*prompts[u]) for u in range(4)]
        for _ in range(3):
            assert sess.poll() == []
        assert [sess.cancel(t) for t in tickets] == ["live"] * 3 + ["pending"]
        idle_after = []
        for _ in range(3):
            assert sess.poll() == []
            idle_after.append(sess.idle)
        assert idle_after == [False, False, True], idle_after
        st = sess.stats()
        assert st["admitted"] == 3 and st["live_rows"] == 3 * 3 * G and sess.cancelled == 4, st
        assert _slots(eng, 3) == [-1] * 3
        assert sess.poll() == [] and sess.idle and sess.stats()["launched_rows"] == st["launched_rows"]
        t6 = sess.submit(*prompts[6])
        got = {t: res for t, res, gen in sess.drain()}
        assert sorted(got) == [t6] and _same(got[t6], want[6])


# ------------------------------------------------------------------------------------------------ 6. editing
def test_an_edit_cancelled_inside_a_span_switch():
    """The three-span edit of tests/test_gpu_session_edit.py's mixed set is cancelled before a batch whose first row step is a fed row of
    one of its span switches (SeqState.feed > 0 when session_cancel_k runs); the TTS request and the one-span edit that share the
    session equal their own oracle runs."""
    from test_gpu_session_edit import engine_for, mixed_requests, row_actions, submit
    args, sd, reqs, want, steps = mixed_requests()
    e3, tts, e1 = 5, 0, 3
    assert len(steps[e3]) == 3 and reqs[tts]["kind"] == "tts" and len(steps[e1]) == 1
    acts = row_actions(steps[e3])
    # row step j >= 1 of a request admitted in front of batch 0 runs in batch (j - 1) // g: the first row step of batch c is 1 + c * g
    place = [(g, c) for g in (3, 2, 4, 5) for c in range(1, len(acts)) if 1 + c * g < len(acts) and acts[1 + c * g] == "F"]
    assert place, steps[e3]
    g, c = place[0]
    eng = engine_for(args, sd, max_seqs=4, max_positions=256)
    eng.set_option("graph_steps", g)
    with eng.open_session(3, top_k=40, stop_repetition=3) as sess:
        tt, t3, t1 = submit(sess, reqs[tts]), submit(sess, reqs[e3]), submit(sess, reqs[e1])
        done = {}
        for _ in range(c):
            done.update({t: res for t, res, gen in sess.poll()})
        assert sess.stats()["turns"] == c and sess.stats()["admitted"] == 3
        assert sess.cancel(t3) == "live"
        done.update({t: res for t, res, gen in sess.drain()})
        assert sorted(done) == sorted([tt, t1]) and sess.idle
        # the rows the cancelled edit really ran: its row steps of batches 0 .. c - 1 (sampled and fed alike), from its record
        ran = c * g
        assert sess.stats()["live_rows"] == ran + (sum(steps[tts]) - 1) + (sum(steps[e1]) - 1), (sess.stats(), ran, steps)
    assert _same(done[tt], want[tts]) and _same(done[t1], want[e1])


# ------------------------------------------------------------------------------------------------ 7. best-of-N
def _group(eng, prompts, u, lo, ctl, hi=10 ** 6):
    """A best-of-3 request on prompt u whose blocking call keeps a sample and takes lo <= n <= hi steps: (seed, res, kept, n)."""
    from test_gpu_session_best_of import blocking
    for seed in range(1, 13):
        res, kept = blocking(eng, prompts[u], 3, seed, ctl, u)
        n = res.shape[2] - prompts[u][2].shape[1] + 4
        if kept >= 0 and lo <= n <= hi:
            return seed, res, kept, n
    raise AssertionError(f"no seed in 1..12 gives prompt {u} a best-of-3 run of {lo}..{hi} steps")


def test_a_group_cancelled_before_it_decides_returns_its_three_slots_together():
    from test_gpu_session_best_of import CTL, _engine as bo_engine, _model
    a, sd, prompts = _model()
    eng = bo_engine(a, sd, max_seqs=4)
    eng.set_option("graph_steps", G)
    s0, _, _, n0 = _group(eng, prompts, 1, 5 + 6 * G, CTL[0])          # its keep decision (step n - 4) lies in batch >= 5
    s1, want1, kept1, _ = _group(eng, prompts, 2, 4, CTL[0])
    c = 2
    with eng.open_session(4, max_samples=3, **CTL[0]) as sess:
        ta = sess.submit(*prompts[1], seed=s0, n_samples=3)
        tb = sess.submit(*prompts[2], seed=s1, n_samples=3)          # one slot is free: it waits for three
        done, admitted = {}, []
        for turn in range(c + 3):
            if turn == c:
                assert sess.stats()["turns"] == c and _slots(eng, 4) == [ta, ta, ta, -1]
                assert sess.cancel(ta) == "live"
            done.update({t: res for t, res, gen in sess.poll()})
            admitted.append(sess.stats()["admitted"])
        assert admitted == [1] * (c + 2) + [2], admitted
        assert _slots(eng, 4) == [tb, tb, tb, -1]
        done.update({t: res for t, res, gen in sess.drain()})
        assert sorted(done) == [tb] and sess.kept == {tb: kept1}
        assert _same(done[tb], want1)


def test_a_group_cancelled_after_it_has_collapsed():
    """The keeper alone is live: the group decided in batch r - 1 (step n - 4), the keeper's last three steps are in batch r, and the
    cancel is made before the turn that queues batch r.  The dropped members have retired by themselves in a batch the host has not
    seen end; the launch leaves them alone and retires the keeper, no layout check fires (the session closes without an error), and
    every slot comes back."""
    from test_gpu_session_best_of import CTL, _engine as bo_engine, _model, blocking
    a, sd, prompts = _model()
    eng = bo_engine(a, sd, max_seqs=4)
    eng.set_option("graph_steps", G)
    s0, _, _, n0 = _group(eng, prompts, 1, 4 + 2 * G, CTL[0])
    r = _last_batch(0, n0)
    assert (n0 - 5) // G == r - 1 and r >= 2
    s1, want1, kept1, _ = _group(eng, prompts, 2, 4, CTL[0])
    wantp, _ = blocking(eng, prompts[3], 1, 7, CTL[0], 3)
    with eng.open_session(4, max_samples=3, **CTL[0]) as sess:
        ta = sess.submit(*prompts[1], seed=s0, n_samples=3)
        for _ in range(r):
            assert sess.poll() == []
        assert sess.stats()["turns"] == r
        assert sess.cancel(ta) == "live"
        for _ in range(3):
            assert sess.poll() == []
        assert sess.idle and _slots(eng, 4) == [-1] * 4
        tb = sess.submit(*prompts[2], seed=s1, n_samples=3)
        tp = sess.submit(*prompts[3], seed=7)
        done = {t: res for t, res, gen in sess.drain()}
        assert sess.stats()["admitted"] == 3
        assert sorted(done) == sorted([tb, tp]) and sess.kept == {tb: kept1}
        assert _same(done[tb], want1) and _same(done[tp], wantp)


def test_a_cancelled_pending_group_at_the_head_of_the_line_lets_the_next_one_in():
    from test_gpu_session_best_of import CTL, _engine as bo_engine, _model, blocking
    a, sd, prompts = _model()
    eng = bo_engine(a, sd, max_seqs=4)
    eng.set_option("graph_steps", G)
    s0, want0, kept0, _ = _group(eng, prompts, 1, 4 + 3 * G, CTL[0])
    wantp, _ = blocking(eng, prompts[3], 1, 7, CTL[0], 3)
    with eng.open_session(4, max_samples=3, **CTL[0]) as sess:
        ta = sess.submit(*prompts[1], seed=s0, n_samples=3)
        tb = sess.submit(*prompts[2], seed=5, n_samples=3)
        tp = sess.submit(*prompts[3], seed=7)
        assert sess.poll() == [] and sess.stats()["admitted"] == 1 and _slots(eng, 4) == [ta, ta, ta, -1]
        assert sess.cancel(tb) == "pending"
        done = {t: res for t, res, gen in sess.poll()}
        assert sess.stats()["admitted"] == 2 and _slots(eng, 4)[3] == tp
        done.update({t: res for t, res, gen in sess.drain()})
        assert sorted(done) == sorted([ta, tp]) and sess.kept == {ta: kept0}
        assert _same(done[ta], want0) and _same(done[tp], wantp)
        assert sess.stats()["admitted"] == 2


# ------------------------------------------------------------------------------------------------ 8. across the wide boundary
def test_cancels_narrow_a_wide_step_and_a_refill_widens_it_again():
    """tiny_h16, twenty live requests on the 17..64-row step.  Requests 2, 3, 16 and 18 are cancelled before the turn that queues batch
    1: the turn that queues batch 3 has sixteen live rows and re-packs to 16.  Four more requests submitted before the next turn widen
    it again.  (The shortest request, 16 steps, has its last step in batch 4: nobody retires by itself before the step has widened.)"""
    eng, prompts, want, n = _tiny(24, max_seqs=20, preset="tiny_h16")
    victims = (2, 3, 16, 18)
    assert _last_batch(0, min(n[:20])) >= 4
    c0 = eng.launch_counts()
    with eng.open_session(20, **GREEDY) as sess:
        tickets = [sess.submit(*p) for p in prompts[:20]]
        done = {t: res for t, res, gen in sess.poll()}
        assert sess.stats()["admitted"] == 20 and sess.stats()["turns"] == 1
        assert [sess.cancel(tickets[u]) for u in victims] == ["live"] * 4
        for _ in range(3):                                   # batches 1, 2 and 3
            done.update({t: res for t, res, gen in sess.poll()})
        st = sess.stats()
        assert done == {} and st["narrowings"] == 1 and st["widenings"] == 0, st
        assert _slots(eng, 20).count(-1) == 4
        tickets += [sess.submit(*p) for p in prompts[20:]]
        done.update({t: res for t, res, gen in sess.poll()})
        st = sess.stats()
        assert st["admitted"] == 24 and st["widenings"] == 1, st
        done.update({t: res for t, res, gen in sess.drain()})
        st = sess.stats()
        assert sess.idle and st["narrowings"] >= 1, st
    c = {k: eng.launch_counts()[k] - c0[k] for k in c0}
    assert c["wd"] > 0, c                                    # the 17..64-row form was in use
    assert sorted(done) == sorted(tickets[u] for u in range(24) if u not in victims)
    for u in range(24):
        if u not in victims:
            assert _same(done[tickets[u]], want[u]), u


# ------------------------------------------------------------------------------------------------ 9. streaming
def test_a_streaming_ticket_cancelled_after_its_second_chunk():
    eng, prompts, want, n = _tiny(6, max_seqs=2)
    chunk = 3
    with eng.open_session(2, **GREEDY) as sess:
        tv, to = sess.submit(*prompts[4], stream=True), sess.submit(*prompts[2], stream=True)
        chunks = {tv: [], to: []}
        done_flag, results, cancelled = set(), {}, False
        for _ in range(200):
            results.update({t: (res, gen) for t, res, gen in sess.poll()})
            for t, first, codes, done in sess.poll_frames(chunk):
                assert not (cancelled and t == tv), "a cancelled ticket got a chunk"
                assert first == sum(ch.shape[1] for ch in chunks[t])
                chunks[t].append(codes[0].cpu().numpy())
                if done:
                    done_flag.add(t)
            if not cancelled and len(chunks[tv]) == 2:
                assert tv not in done_flag
                assert sess.cancel(tv) == "live"
                cancelled = True
            if sess.idle:
                break
        assert cancelled and sess.idle and sess.poll_frames(chunk) == []
        assert sorted(results) == [to] and done_flag == {to}
    K = 4
    gen_v = want[4][0][:, prompts[4][2].shape[1]:]
    got_v = np.concatenate(chunks[tv], axis=1)
    assert chunk * 2 <= got_v.shape[1] < gen_v.shape[1] and np.array_equal(got_v, gen_v[:, : got_v.shape[1]])
    got_o = np.concatenate(chunks[to], axis=1)
    assert np.array_equal(got_o, results[to][1][0].cpu().numpy()) and _same(results[to][0], want[2])


def test_session_streamer_cancel_returns_the_codec_stream_id():
    from _util import build_case
    from voicecraft_amd import SessionStreamer, synth
    from voicecraft_amd.codec import AudioTokenizer
    from voicecraft_amd.engine import VoiceCraftEngine
    _, args, sd, _, _, _ = build_case("tts_greedy")                         # the model of tests/test_gpu_session_audio.py
    eng = VoiceCraftEngine(args, sd, device="cuda:0", dtype="fp32", max_seqs=2, max_positions=256)
    eng.set_option("graph_steps", G)
    tok = AudioTokenizer(synth.make_codec_state_dict(0), device="cuda:0", max_seconds=8.0, max_batch=2)
    prompts = [synth.random_prompt(args, 4 + u, 12 + 5 * u, seed=1300 + u) for u in (3, 1, 2)]
    audio, ids_seen = {}, {}
    with eng.open_session(2, top_k=1, stop_repetition=3) as sess:
        pump = SessionStreamer(sess, tok, chunk_frames=3)
        tv, to = sess.submit(*prompts[0], stream=True), sess.submit(*prompts[1], stream=True)
        tn = None
        for _ in range(400):
            for t, wav, done in pump.pump():
                assert t != tv or tn is None, "a cancelled ticket got audio"
                audio.setdefault(t, []).append(wav)
            ids_seen.update(pump.ids)
            if tn is None and len(audio.get(tv, [])) >= 2:
                sid = pump.ids[tv]
                assert to in pump.ids, "precondition: the other ticket is still streaming, so the free list is empty"
                assert pump.cancel(tv) == "live" and tv not in pump.ids and sid in pump.free
                tn = sess.submit(*prompts[2], stream=True)
            if tn is not None and sess.idle and not pump.ids:
                break
        results = {t: (res, gen) for t, res, gen in pump.take_results()}
        assert sess.idle and sorted(results) == sorted([to, tn]) and sorted(pump.free) == [0, 1]
        assert ids_seen[tn] == ids_seen[tv] != ids_seen[to], ids_seen      # the cancelled ticket's stream id carried the later ticket
    for t in (to, tn):
        gen = results[t][1]
        assert int(gen.min()) >= 0 and int(gen.max()) < 2048, "precondition: the requests generate codec ids only"
        wav_want = tok.decode([(gen, None)])
        got = torch.cat(audio[t], dim=2)
        assert got.shape == wav_want.shape and torch.equal(got, wav_want), (t, got.shape, wav_want.shape)


# ------------------------------------------------------------------------------------------------ 10. reproducible in bf16
def _bf16_schedule(eng, prompts, seeds):
    """Six live on eight rows; three of them cancelled before batch 2, so that the turn that queues batch 4 narrows to 4 rows; five more
    submitted then (the step widens), one of them cancelled while pending and one while live; the rest at the end."""
    tickets, done = [], {}
    with eng.open_session(6, top_k=40, stop_repetition=3) as sess:
        def submit(lo, hi):
            for u in range(lo, hi):
                tickets.append(sess.submit(*prompts[u], seed=seeds[u]))

        def poll(k):
            for _ in range(k):
                for t, res, gen in sess.poll():
                    done[t] = res.cpu().numpy()
        submit(0, 6)
        poll(2)
        was = [sess.cancel(tickets[u]) for u in (1, 2, 4)]
        poll(3)
        mid = sess.stats()
        submit(6, 11)
        was.append(sess.cancel(tickets[9]))
        poll(2)
        was.append(sess.cancel(tickets[7]))
        submit(11, len(prompts))
        while not sess.idle:
            poll(1)
        return tickets, done, was, mid, sess.stats(), sess.cancelled


def test_bf16_tokens_and_counters_are_a_function_of_the_schedule():
    n = 14
    a, sd, prompts = _workload("tiny128", n)
    eng = _engine(a, sd, "bf16", 8)
    eng.set_option("graph_steps", G)
    seeds = [100 + u for u in range(n)]
    runs = []
    for i in range(6):
        if i % 2:
            time.sleep(0.02 * i)                      # another phase between the host's loop and the device's
        runs.append(_bf16_schedule(eng, prompts, seeds))
    tickets, done, was, mid, st, cancelled = runs[0]
    assert was == ["live", "live", "live", "pending", "live"] and cancelled == 5, was
    assert mid["narrowings"] >= 1 and st["widenings"] >= 1 and st["admitted"] == n - 1, (mid, st)
    gone = {tickets[u] for u in (1, 2, 4, 9, 7)}
    assert sorted(done) == sorted(t for t in tickets if t not in gone)
    assert len({r.shape[2] for r in done.values()}) > 1
    for i in range(1, 6):
        ti, di, wi, mi, si, ci = runs[i]
        assert (wi, mi, si, ci) == (was, mid, st, cancelled), (i, si, st)
        assert sorted(di) == sorted(done)
        for t in done:
            assert di[t].shape == done[t].shape and np.array_equal(di[t], done[t]), (i, t)


# ------------------------------------------------------------------------------------------------ 11. the one-shot path
def test_the_one_shot_call_is_untouched_by_a_session_with_cancels():
    eng, prompts, want, n = _tiny(6, max_seqs=3)
    x, xl, y = (v.cuda() for v in prompts[0])
    before = eng.inference_tts(x, xl, y, top_k=40, stop_repetition=3, _seed=5)[0].cpu().numpy()
    with eng.open_session(3, top_k=40, stop_repetition=3) as sess:
        tickets = [sess.submit(*prompts[u], seed=u) for u in range(5)]
        sess.poll()
        sess.poll()
        assert [sess.cancel(tickets[u]) for u in (0, 3)] == ["live", "pending"]
        sess.drain()
        assert sess.cancelled == 2
    after = eng.inference_tts(x, xl, y, top_k=40, stop_repetition=3, _seed=5)[0].cpu().numpy()
    assert after.shape == before.shape and np.array_equal(after, before)
