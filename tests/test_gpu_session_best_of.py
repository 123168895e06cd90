"""-m gpu: best-of-N TTS requests in a decode session (include/vc_engine.h vc_session_open_best_of, vc_session_submit_best_of,
vc_session_kept).  A request of N samples is one ticket, N rows and N K/V slots; its prompt is prefilled once and replicated; the LAST
sample whose first codebook terminates first is kept.  In exact mode every request - tokens AND kept index - must be its own blocking
call inference_tts_multi([x], [y], batch_size=N, _seed=s) of the same engine (parent code, pinned to the reference by draw replay in
tests/test_gpu_tts_best_of.py), whatever slots it landed in and whatever it shared a step with.  Every comparison is bit equality."""
import time

import numpy as np
import pytest
import torch

from test_gpu_session import _drain_collecting_failures, _workload

pytestmark = pytest.mark.gpu

TERM = 2051
# two control sets.  The synthetic checkpoint's logits are tight (sigma ~ 0.15), so a terminator boost of 0.2 already makes it likely
# enough to be DRAWN on some step after min_gen while the arg-max rule stays quiet: the blocking calls of the seeds used below end after
# 11 .. 80 steps and keep samples 0, 1 and 2 (a boost of 0.8 or more makes the terminator the arg-max: every group then ends on step
# min_gen + 1 with all samples tied)
CTL = (dict(top_k=0, top_p=0.95, temperature=1.0, stop_repetition=2), dict(top_k=40, top_p=1.0, temperature=1.2, stop_repetition=3))
W_STATE = 16 + 2 * 8 + 3            # SeqState in 4-byte words (vc_common.h; VC_MAX_SPANS = 8)
I_DONE, I_GROUP, I_SLOT = 8, 14, 32


def _model(preset="tiny", boost=0.2):
    from voicecraft_amd import synth
    a = synth.make_args(preset)
    sd = synth.make_state_dict(a, seed=3, mute_eos=False, boost=[(0, TERM, boost)])
    prompts = [synth.random_prompt(a, 7 + (u % 6), 20 + 4 * (u % 6), seed=900 + u) for u in range(8)]
    return a, sd, prompts


def _engine(a, sd, dtype="fp32", max_seqs=8, graph=True, max_positions=256):
    from voicecraft_amd.engine import VoiceCraftEngine
    return VoiceCraftEngine(a, sd, device="cuda:0", dtype=dtype, max_seqs=max_seqs, max_positions=max_positions, use_graph=graph)


_WANT = {}       # blocking results, computed once per (engine, request) and left unchanged


def blocking(eng, prompt, N, seed, ctl, tag):
    """(res as numpy, kept index) of the request's own blocking call on `eng`."""
    key = (id(eng), tag, N, seed, tuple(sorted(ctl.items())))
    if key not in _WANT:
        x, xl, y = prompt
        if N == 1:
            res = eng.inference_tts(x.cuda(), xl.cuda(), y.cuda(), _seed=seed, **ctl)[0]
            _WANT[key] = (res.cpu().numpy(), 0)
        else:
            out = eng.inference_tts_multi([x[0]], [y[0]], batch_size=N, _seed=seed, **ctl)
            _WANT[key] = (out[0][0].cpu().numpy(), int(eng.last_kept[0]))
    return _WANT[key]


def assert_exercises_the_rule(wants, prompts_T, Ns):
    """The blocking results the session is compared with: kept indices of at least two values, one of them not N - 1, lengths differ."""
    kept = [k for (_, k), N in zip(wants, Ns) if N > 1]
    assert len(set(kept)) >= 2, kept
    assert any(k != N - 1 for (_, k), N in zip(wants, Ns) if N > 1), (kept, Ns)
    lens = [r.shape[2] - T for (r, _), T in zip(wants, prompts_T)]
    assert len(set(lens)) >= 2, lens


def lone(eng, prompt, N, seed, ctl):
    x, xl, y = prompt
    with eng.open_session(N, max_samples=N, **ctl) as sess:
        t = sess.submit(x, xl, y, seed=seed, n_samples=N)
        done = {tt: r for tt, r, g in sess.drain()}
        return done[t].cpu().numpy(), sess.kept[t], sess.stats()


# ------------------------------------------------------------------------------------------------ 1. greedy against the oracle
@pytest.mark.parametrize("N", [3, 2, 4])
def test_greedy_fp32_equals_the_oracles_inference_tts_batch(N):
    """top_k = 1: all samples are equal, so sample N - 1 is kept - and it decoded entirely on COPIED prompt K/V."""
    from oracle.voicecraft_oracle import VoiceCraftOracle
    a, sd, prompts = _workload("tiny", 3)
    torch.set_num_threads(min(4, torch.get_num_threads()))
    orc = VoiceCraftOracle(a, sd)
    eng = _engine(a, sd, max_seqs=4)
    for (x, xl, y) in prompts[:2]:
        want = orc.inference_tts_batch(x, xl, y, batch_size=N, top_k=1, stop_repetition=3)[0].numpy()
        with eng.open_session(N, max_samples=N, top_k=1, stop_repetition=3) as sess:
            t = sess.submit(x, xl, y, seed=1, n_samples=N)
            done = {tt: r for tt, r, g in sess.drain()}
            assert sess.kept[t] == N - 1, sess.kept
        got = done[t].cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (N, got.shape, want.shape)


# ------------------------------------------------------------------------------------------------ 2. sibling K/V
def _copy_chunk_rows(esz, hd):
    """Positions one pass of copy_kv_k's grid covers per head: gridDim.x = 8 workgroups of 256 threads, 16 bytes each."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voicecraft_amd", "csrc", "vc_attn.hip")).read()
    m = re.search(r"copy_kv_k<uint4>, dim3\((\d+), a\.H, a\.n_dst\), dim3\((\d+)\)", src)
    assert m, "copy_kv_k's launch geometry is not where this test reads it"
    return int(m.group(1)) * int(m.group(2)) * 16 // (hd * esz)


@pytest.mark.parametrize("dtype,preset", [("fp32", "tiny"), ("bf16", "tiny128")])
def test_sibling_kv_is_the_prompts_bit_for_bit(dtype, preset):
    from voicecraft_amd import synth
    a, sd, _ = _model(preset)
    N = 3
    H, hd = a.nhead, a.d_model // a.nhead
    esz = 4 if dtype == "fp32" else 2
    chunk = _copy_chunk_rows(esz, hd)            # prompt rows (positions) per grid pass
    assert 16 <= chunk <= 200, chunk
    eng = _engine(a, sd, dtype, max_seqs=N)
    # a row count that is a multiple of the per-pass chunk, one that is not (and is more than one pass), and a short one
    for rows in (chunk, chunk + 5, 37):
        Lx = 9
        T = rows - Lx - 1
        assert T >= 1
        x, xl, y = synth.random_prompt(a, Lx, T, seed=77 + rows)
        with eng.open_session(N, max_samples=N, top_k=1, stop_repetition=3) as sess:
            t = sess.submit(x, xl, y, seed=3, n_samples=N)
            sess.poll()
            slots = eng.debug_read("session_slots", (N + 1,), torch.int32).tolist()
            assert slots[1:] == [t] * N, slots
            sess.drain()
        for l in range(a.num_decoder_layers):
            for name in ("kcache", "vcache"):
                if dtype == "fp32":
                    c = eng.debug_read(f"{name}{l}", (N, H, 256, hd), torch.float32).view(torch.int32)
                else:
                    c = eng.debug_read(f"{name}{l}", (N, H, 256, hd), torch.int16)
                assert bool((c[0, :, :rows] != 0).any())
                for j in range(1, N):
                    assert torch.equal(c[j, :, :rows], c[0, :, :rows]), (dtype, rows, l, name, j)


# ------------------------------------------------------------------------------------------------ 3. a lone sampled request
LONE_SEEDS = (1, 2, 3, 4, 5, 6)


@pytest.mark.parametrize("graph", [True, False])
def test_a_lone_sampled_request_equals_its_blocking_call(graph):
    a, sd, prompts = _model()
    eng = _engine(a, sd, graph=graph)
    cases = [(N, s, 1 + (s % 2)) for N in (2, 3, 4) for s in LONE_SEEDS]
    wants = [blocking(eng, prompts[u], N, s, CTL[0], u) for N, s, u in cases]
    assert_exercises_the_rule(wants, [prompts[u][2].shape[1] for _, _, u in cases], [N for N, _, _ in cases])
    for (N, s, u), (want, wk) in zip(cases, wants):
        got, gk, st = lone(eng, prompts[u], N, s, CTL[0])
        print(N, s, u, "kept", gk, wk, "len", got.shape[2], want.shape[2], st)
        assert gk == wk, (N, s, gk, wk)
        assert got.shape == want.shape and np.array_equal(got, want), (N, s, got.shape, want.shape)
        assert st["admitted"] == 1 and st["live_rows"] <= st["launched_rows"], st


# ------------------------------------------------------------------------------------------------ 4. / 8. the mixed schedule
def _mixed_requests(a, prompts):
    """(kind, prompt index, N, seed, control set, spans) - plain TTS, one-span edits, best-of-2 and best-of-3."""
    from voicecraft_amd import synth
    # wave 1 takes slots 0..3; the requests in slots 1 and 3 are short (13 and 12 steps), those in 0 and 2 long (50 and 62): by the
    # time the best-of-3 of wave 2 reaches the head of the queue, slots 1, 3 and 7 are the free ones, and it lives for 67 steps behind
    # rows that retire before it
    R = [("tts", 0, 1, 0, 0, None), ("tts", 3, 1, 9, 1, None), ("tts", 2, 1, 0, 0, None), ("tts", 1, 1, 0, 0, None),      # wave 1
         ("bo", 4, 2, 1, 0, None), ("edit", 5, 1, 22, 1, [(8, 14)]), ("bo", 3, 3, 8, 0, None), ("tts", 2, 1, 5, 1, None),  # wave 2
         ("bo", 1, 3, 2, 1, None), ("edit", 0, 1, 32, 0, [(5, 11)]), ("bo", 5, 2, 3, 1, None), ("tts", 4, 1, 7, 0, None),
         ("bo", 2, 2, 4, 0, None), ("bo", 0, 3, 0, 1, None)]                                                              # wave 3
    return R


def _edit_ctl(c):
    return dict(CTL[c], stop_repetition=-1)


def _submit(sess, r, prompts):
    kind, u, N, seed, c, spans = r
    x, xl, y = prompts[u]
    if kind == "edit":
        return sess.submit_edit(x, xl, y, torch.tensor([spans], dtype=torch.int64), seed=seed, **_edit_ctl(c))
    return sess.submit(x, xl, y, seed=seed, n_samples=N, **CTL[c])


def _want(eng, r, prompts):
    kind, u, N, seed, c, spans = r
    if kind == "edit":
        key = (id(eng), "edit", u, seed, c)
        if key not in _WANT:
            x, xl, y = prompts[u]
            res = eng.inference_multi([x[0]], [y[0]], [list(spans)], _seed=seed, **_edit_ctl(c))
            _WANT[key] = (res[0].cpu().numpy(), 0)
        return _WANT[key]
    return blocking(eng, prompts[u], N, seed, CTL[c], u)


def _mixed_run(eng, prompts, reqs, max_live=8, watch=False):
    """Three waves between polls (the pattern of test_gpu_session._scheduled_run).  watch: after every poll, the slot table and the
    live rows (group, slot) of the step in force, read from the session's bookkeeping and the device state."""
    tickets, done, trace = [], {}, []
    NS = eng.max_seqs
    with eng.open_session(max_live, max_samples=3, **CTL[0]) as sess:
        def poll():
            for t, res, gen in sess.poll():
                done[t] = res.cpu().numpy()
            if watch:
                sl = eng.debug_read("session_slots", (max_live + 1,), torch.int32).tolist()
                st = eng.debug_read("state", (NS, W_STATE), torch.int32)
                rows = [(int(st[r, I_GROUP]), int(st[r, I_SLOT])) if not int(st[r, I_DONE]) else None for r in range(sl[0])]
                trace.append((sl[1:], rows))
        for r in reqs[:4]:
            tickets.append(_submit(sess, r, prompts))
        for _ in range(3):
            poll()
        for r in reqs[4:8]:
            tickets.append(_submit(sess, r, prompts))
        for _ in range(2):
            poll()
        for r in reqs[8:]:
            tickets.append(_submit(sess, r, prompts))
        while not sess.idle:
            poll()
        stats, kept = sess.stats(), dict(sess.kept)
    return [done[t] for t in tickets], [kept.get(t, 0) for t in tickets], tickets, stats, trace


def test_mixed_schedule_every_request_equals_its_own_blocking_call():
    a, sd, prompts = _model()
    eng = _engine(a, sd, max_seqs=8)
    reqs = _mixed_requests(a, prompts)
    wants = [_want(eng, r, prompts) for r in reqs]
    bo = [i for i, r in enumerate(reqs) if r[0] == "bo"]
    assert_exercises_the_rule([wants[i] for i in bo], [prompts[reqs[i][1]][2].shape[1] for i in bo], [reqs[i][2] for i in bo])
    got, kept, tickets, stats, trace = _mixed_run(eng, prompts, reqs, watch=True)
    print(stats, kept)
    for i, (r, (want, wk)) in enumerate(zip(reqs, wants)):
        assert kept[i] == wk, (i, r, kept[i], wk)
        assert got[i].shape == want.shape and np.array_equal(got[i], want), (i, r, got[i].shape, want.shape)
    assert stats["admitted"] == len(reqs) and stats["admitted_while_live"] >= 1, stats
    assert stats["widenings"] >= 1 and stats["narrowings"] >= 1, stats
    assert 0 < stats["live_rows"] <= stats["launched_rows"], stats
    # a group in non-consecutive slots: from the session's slot table
    groups = {t for t, r in zip(tickets, reqs) if r[0] == "bo"}
    split = False
    for slots, _ in trace:
        for t in groups:
            mine = [s for s, tt in enumerate(slots) if tt == t]
            split |= len(mine) >= 2 and mine[-1] - mine[0] != len(mine) - 1
    assert split, [s for s, _ in trace]
    # a group whose rows moved together: all its members live on consecutive rows in two consecutive polls, further to the front in
    # the second, which only a retired row in front of them makes happen
    moved = False
    for (_, r0), (_, r1) in zip(trace, trace[1:]):
        for t in groups:
            p0 = [i for i, v in enumerate(r0) if v is not None and v[0] == t]
            p1 = [i for i, v in enumerate(r1) if v is not None and v[0] == t]
            n = next(r[2] for tt, r in zip(tickets, reqs) if tt == t)
            if len(p0) == n and len(p1) == n and p1[0] < p0[0]:
                assert [i - p0[0] for i in p0] == list(range(n)) and [i - p1[0] for i in p1] == list(range(n)), (t, p0, p1)
                assert [r1[i][1] for i in p1] == [r0[i][1] for i in p0]          # the same slots, in sample order
                moved = True
    assert moved, [r for _, r in trace]


def test_bf16_tokens_kept_indices_and_stats_are_the_same_in_every_run():
    a, sd, prompts = _model("tiny128")
    eng = _engine(a, sd, "bf16", max_seqs=8)
    eng.set_option("graph_steps", 3)
    reqs = _mixed_requests(a, prompts)
    runs = []
    for i in range(6):
        if i % 2:
            time.sleep(0.02 * i)                      # another phase between the host's loop and the device's
        got, kept, _, stats, _ = _mixed_run(eng, prompts, reqs)
        runs.append((got, kept, stats))
    assert len({g.shape[2] for g in runs[0][0]}) > 1
    assert runs[0][2]["admitted_while_live"] >= 1 and runs[0][2]["widenings"] + runs[0][2]["narrowings"] >= 1, runs[0][2]
    for i in range(1, 6):
        assert runs[i][2] == runs[0][2], (i, runs[i][2], runs[0][2])
        assert runs[i][1] == runs[0][1], (i, runs[i][1], runs[0][1])
        for u in range(len(reqs)):
            assert runs[i][0][u].shape == runs[0][0][u].shape and np.array_equal(runs[i][0][u], runs[0][0][u]), (i, u)


# ------------------------------------------------------------------------------------------------ 5. head-of-line blocking
def test_a_group_waiting_for_slots_blocks_the_line():
    a, sd, prompts = _model()
    eng = _engine(a, sd, max_seqs=8)
    order = [("tts", 0, 1, 3, 0, None), ("tts", 1, 1, 2, 1, None), ("tts", 2, 1, 0, 0, None), ("bo", 3, 3, 0, 0, None),
             ("tts", 4, 1, 2, 1, None), ("tts", 5, 1, 8, 0, None)]
    wants = [_want(eng, r, prompts) for r in order]
    done, adm, seen = {}, [], set()
    with eng.open_session(5, max_samples=3, **CTL[0]) as sess:
        tickets = [_submit(sess, r, prompts) for r in order]
        while not sess.idle:
            for t, res, gen in sess.poll():
                done[t] = res.cpu().numpy()
            slots = eng.debug_read("session_slots", (6,), torch.int32).tolist()[1:]
            seen |= {t for t in slots if t >= 0}
            # nobody submitted behind the group holds a slot before the group does
            assert tickets[3] in seen or not ({tickets[4], tickets[5]} & seen), (slots, tickets)
            adm.append((sess.stats()["admitted"], slots.count(-1)))
        kept = dict(sess.kept)
    # FIFO: the first turn admits the three plain requests and leaves two slots free - for the group's three samples that is one too
    # few, and the two plain requests behind it are NOT admitted into them
    assert adm[0] == (3, 2), adm
    stuck = [n for n, free in adm if n == 3]
    assert len(stuck) >= 2, adm                       # (at least one more turn went by with two slots free and nobody admitted)
    counts = [n for n, _ in adm]
    assert counts == sorted(counts) and counts[-1] == 6, adm
    first4 = next(n for n in counts if n > 3)
    assert first4 >= 4, adm                           # the group goes first; the later ones with it or after it, never before
    for t, (want, wk), r in zip(tickets, wants, order):
        assert kept.get(t, 0) == wk, (r, kept.get(t, 0), wk)
        assert done[t].shape == want.shape and np.array_equal(done[t], want), r


# ------------------------------------------------------------------------------------------------ 6. ties and a first-step decision
def test_simultaneous_terminators_keep_the_last_of_them():
    """Sessions take no forced draws, so a tie is looked for among 32 seeds with blocking calls alone.  Sample j of a best-of-N call
    draws on (seed, sequence j), whatever N is, and fp32 logits do not depend on the batch: the best-of-2 call of a seed is samples 0
    and 1 of its best-of-3 call, the one-sample call is sample 0.  Kept 2 with a best-of-2 call of the same length: sample 0 or 1
    terminates on the step sample 2 does.  Kept 1 with a one-sample call of the same length: samples 0 and 1 terminate together."""
    a, sd, prompts = _model()
    eng = _engine(a, sd, max_seqs=8)
    u, ctl = 4, CTL[1]
    found = None
    for seed in range(100, 132):
        want, wk = blocking(eng, prompts[u], 3, seed, ctl, u)
        if wk == 2 and blocking(eng, prompts[u], 2, seed, ctl, u)[0].shape[2] == want.shape[2]:
            found = (seed, want, wk)
        elif wk == 1 and blocking(eng, prompts[u], 1, seed, ctl, u)[0].shape[2] == want.shape[2]:
            found = (seed, want, wk)
        if found:
            break
    if found is None:
        pytest.skip("none of the 32 seeds makes two samples of a best-of-3 call terminate on the same step")
    seed, want, wk = found
    print("tie: seed", seed, "kept", wk, "frames", want.shape[2] - prompts[u][2].shape[1])
    got, gk, _ = lone(eng, prompts[u], 3, seed, ctl)
    assert gk == wk and got.shape == want.shape and np.array_equal(got, want)


def test_a_group_decided_at_the_first_possible_step_and_by_its_first_sample():
    """A terminator boosted far above everything: the arg-max rule fires for every sample on step min_gen + 1, all N terminate together
    and the last is kept.  And a prompt already past its length cap (y_len > cap_len at the first sample): the group is decided by
    the FIRST forms of the sampler pair."""
    from voicecraft_amd import synth
    a, sd, prompts = _model(boost=30.0)
    eng = _engine(a, sd, max_seqs=8)
    min_gen = a.encodec_sr // 5
    want, wk = blocking(eng, prompts[1], 3, 5, CTL[0], "argmax")
    assert wk == 2 and want.shape[2] - prompts[1][2].shape[1] == min_gen + 1, (wk, want.shape)
    got, gk, _ = lone(eng, prompts[1], 3, 5, CTL[0])
    assert gk == 2 and got.shape == want.shape and np.array_equal(got, want)
    short = synth.random_prompt(a, 3, 35, seed=5)                  # cap_len = 30 < 36 columns
    want, wk = blocking(eng, short, 3, 6, CTL[0], "cap")
    assert wk == 2 and want.shape[2] == 35, (wk, want.shape)      # the terminator on the first step: no frame generated
    got, gk, _ = lone(eng, short, 3, 6, CTL[0])
    assert gk == 2 and got.shape == want.shape and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ 7. the wide step
def test_wide_step_five_best_of_four():
    a, sd, prompts = _model("tiny_h16")
    eng = _engine(a, sd, max_seqs=20)
    reqs = [("bo", u, 4, u, u % 2, None) for u in range(5)]
    wants = [_want(eng, r, prompts) for r in reqs]
    c0 = eng.launch_counts()
    with eng.open_session(20, max_samples=4, **CTL[0]) as sess:
        tickets = [_submit(sess, r, prompts) for r in reqs]
        done = {t: res.cpu().numpy() for t, res, gen in sess.drain()}
        kept, stats = dict(sess.kept), sess.stats()
    c = {k: eng.launch_counts()[k] - c0[k] for k in c0}
    assert c["wd"] > 0, c                              # the 17..64-row form was in use
    assert stats["admitted"] == 5 and stats["launched_rows"] >= 32, stats
    for t, (want, wk), r in zip(tickets, wants, reqs):
        assert kept[t] == wk, (r, kept[t], wk)
        assert done[t].shape == want.shape and np.array_equal(done[t], want), r


# ------------------------------------------------------------------------------------------------ 9. refusals and recovery
def test_refusals_and_recovery():
    import ctypes as C
    from voicecraft_amd._lib import EngineError
    a, sd, prompts = _model()
    eng = _engine(a, sd, max_seqs=8)
    x, xl, y = prompts[0]
    before_multi = blocking(eng, prompts[0], 3, 9, CTL[0], 0)
    before_plain = eng.inference_tts_queue([x[0]], [y[0]], max_live=2, seeds=[9], **CTL[0])[0][0].cpu().numpy()
    with pytest.raises(AssertionError, match="max_samples"):
        eng.open_session(2, max_samples=3)
    with eng.open_session(4, **CTL[0]) as sess:                   # opened without max_samples
        with pytest.raises(AssertionError, match=r"n_samples 2 outside \[1, max_samples = 1\]"):
            sess.submit(x, xl, y, n_samples=2)
        xd, Lx, yd, T = sess._upload(x, xl, y)
        t = C.c_int(0)
        rc = eng.lib.vc_session_submit_best_of(eng._h, C.c_void_p(xd.data_ptr()), Lx, C.c_void_p(yd.data_ptr()), T, 2, None, 0, C.byref(t))
        assert rc == -1 and b"n_samples 2" in eng.lib.vc_last_error(eng._h) and b"max_samples = 1" in eng.lib.vc_last_error(eng._h)
        t0 = sess.submit(x, xl, y, seed=9)                        # ... and the session goes on
        assert np.array_equal({tt: r for tt, r, g in sess.drain()}[t0].cpu().numpy(), before_plain)
    with eng.open_session(5, max_samples=3, **CTL[0]) as sess:
        for n in (4, 0, -1):
            with pytest.raises(AssertionError, match="max_samples = 3"):
                sess.submit(x, xl, y, n_samples=n)
            rc = eng.lib.vc_session_submit_best_of(eng._h, C.c_void_p(xd.data_ptr()), Lx, C.c_void_p(yd.data_ptr()), T, n, None, 0, C.byref(t))
            assert rc == -1 and f"n_samples {n}".encode() in eng.lib.vc_last_error(eng._h)
        with pytest.raises(AssertionError, match="best-of-N requests do not stream"):
            sess.submit(x, xl, y, n_samples=2, stream=True)
        with pytest.raises(AssertionError, match="not supported per request"):
            sess.submit_edit(x, xl, prompts[0][2], torch.tensor([[[5, 9]]]), n_samples=2)
        tb = sess.submit(x, xl, y, seed=9, n_samples=3)
        with pytest.raises(AssertionError, match="best-of-N requests do not stream"):
            sess._frames([tb], 1)                                  # (what poll_frames calls for the tickets marked as streaming)
        # an out-of-range id in a best-of-3 prompt: reported for its ticket, and all three slots come back
        bad_y = prompts[1][2].clone()
        bad_y[0, 3, 2] = 5000
        t_bad = sess.submit(prompts[1][0], prompts[1][1], bad_y, seed=4, n_samples=3)
        got, failed = _drain_collecting_failures(sess)
        assert sorted(failed) == [t_bad] and f"ticket {t_bad}" in str(failed[t_bad]) and "out of range" in str(failed[t_bad]), failed
        done = {tt: r.cpu().numpy() for tt, r, g in got}
        assert sess.kept[tb] == before_multi[1] and np.array_equal(done[tb], before_multi[0])
        assert eng.debug_read("session_slots", (6,), torch.int32).tolist()[1:] == [-1] * 5
        adm = sess.stats()["admitted"]
        for u in (2, 3, 4, 5, 0):
            sess.submit(*prompts[u], seed=u)
        sess.poll()
        assert sess.stats()["admitted"] == adm + 5                 # five plain requests in ONE turn: every slot was free
        sess.drain()
    # after close the blocking best-of-N call and a plain session give what they gave before
    _WANT.clear()
    again = blocking(eng, prompts[0], 3, 9, CTL[0], 0)
    assert again[1] == before_multi[1] and np.array_equal(again[0], before_multi[0])
    plain = eng.inference_tts_queue([x[0]], [y[0]], max_live=2, seeds=[9], **CTL[0])[0][0].cpu().numpy()
    assert np.array_equal(plain, before_plain)


def test_a_group_that_runs_out_of_positions_fails_alone():
    """No sample of the group terminates within max_positions: VC_ECAP at fetch, with the blocking call's words, and the requests
    decoded next to it keep their results."""
    from voicecraft_amd._lib import EngineError
    from voicecraft_amd import synth
    a = synth.make_args("tiny")
    sd = synth.make_state_dict(a, seed=3)                          # muted terminator: a request ends on its length cap only
    prompts = [synth.random_prompt(a, 4, 30, seed=1), synth.random_prompt(a, 12, 30, seed=2), synth.random_prompt(a, 4, 28, seed=3)]
    eng = _engine(a, sd, max_seqs=8, max_positions=96)             # 12 phonemes: cap 120 columns > 96 positions; 4 phonemes: 40
    with pytest.raises(EngineError, match="no sample terminated"):
        eng.inference_tts_multi([prompts[1][0][0]], [prompts[1][2][0]], batch_size=3, _seed=2, **CTL[0])
    wants = [blocking(eng, prompts[u], N, 7 + u, CTL[0], ("cap", u)) for u, N in ((0, 2), (2, 1))]
    with eng.open_session(6, max_samples=3, **CTL[0]) as sess:
        t0 = sess.submit(*prompts[0], seed=7, n_samples=2)
        tb = sess.submit(*prompts[1], seed=2, n_samples=3)
        t2 = sess.submit(*prompts[2], seed=9)
        got, failed = _drain_collecting_failures(sess)
        assert sorted(failed) == [tb] and isinstance(failed[tb], EngineError), failed
        assert f"ticket {tb}" in str(failed[tb]) and "no sample terminated within the step budget" in str(failed[tb])
        done = {tt: r.cpu().numpy() for tt, r, g in got}
        assert np.array_equal(done[t0], wants[0][0]) and sess.kept[t0] == wants[0][1]
        assert np.array_equal(done[t2], wants[1][0])
        assert eng.debug_read("session_slots", (7,), torch.int32).tolist()[1:] == [-1] * 6


# ------------------------------------------------------------------------------------------------ 10. the queue helper
def test_inference_tts_queue_best_of_three():
    a, sd, prompts = _model()
    eng = _engine(a, sd, max_seqs=8)
    us = [0, 1, 2, 3, 4, 5, 1]
    seeds = [1, 1, 2, 3, 4, 5, 6]
    wants = [blocking(eng, prompts[u], 3, s, CTL[1], u) for u, s in zip(us, seeds)]
    assert_exercises_the_rule(wants, [prompts[u][2].shape[1] for u in us], [3] * 7)
    got = eng.inference_tts_queue([prompts[u][0][0] for u in us], [prompts[u][2][0] for u in us], max_live=8, seeds=seeds, batch_size=3,
                                  **CTL[1])
    assert eng.last_kept == [k for _, k in wants], (eng.last_kept, [k for _, k in wants])
    for (res, gen), (want, _), u in zip(got, wants, us):
        r = res.cpu().numpy()
        assert r.shape == want.shape and np.array_equal(r, want)
        assert np.array_equal(gen.cpu().numpy(), want[:, :, prompts[u][2].shape[1]:])
    st = eng.last_session_stats
    assert st["admitted"] == 7 and st["admitted_while_live"] >= 1, st
