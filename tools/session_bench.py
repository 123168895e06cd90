"""Decode sessions (continuous batching) against what the blocking API offers for the same work, on ONE engine, interleaved pairs:
python tools/session_bench.py [--preset giga830M] [--pairs 5] [--sizes 64:8,256:64] [--edit-share 0.5] [--best-of 3 --sizes 48:24]

Workload: the ragged utterances of bench.py's ragged_block (giga830M shape, bf16, top-k 40, 150 prompt frames, the synthetic
checkpoint's terminator muted, so an utterance of Lx phonemes ends at the reference's length cap: 10 Lx - 150 generated frames).  `N:L`
= N utterances through L slots; utterance u has the phoneme count of ragged_block's utterance u mod L (40 .. 80, evenly spread), so
every consecutive group of L utterances is exactly that block's batch.
  * baseline: inference_tts_multi on consecutive groups of L utterances in input order - each call runs until its longest member ends;
  * session:  inference_tts_queue(max_live = L) - a freed slot is refilled with the next utterance while the others go on decoding.
Per size one JSON line: codec-tokens/s of both arms (median, min, max over the pairs) and the per-pair ratio; the mean number of live
rows per launched step and the share of launched rows that were live (session: its own counters; baseline: from the utterances' step
counts, with the launched rows simulated from the blocking loop's re-pack rule); the decode-stream time per admitted request (prefill +
re-pack + first sample, HIP events).  Both arms produce the same number of frames per utterance (asserted).
--edit-share F: that fraction of the requests (evenly spread) are one-span editing requests with the editing front-end's defaults
(top_k 0, top_p 0.8, stop_repetition -1; the span covers the middle third of the prompt frames), submitted to the SAME session with
their own controls next to the TTS requests.  The baseline then runs, for every consecutive group of L requests, inference_tts_multi on
the group's TTS requests and inference_multi on its editing requests - what the blocking API offers when the two kinds cannot share a
step; the frames compared and counted are the generated ones of either kind.
--best-of B (B > 1; TTS only): every utterance is a best-of-B request.  `N:L` = N utterances through L slots, L a multiple of B:
  * baseline: consecutive inference_tts_multi(batch_size=B) calls of L / B utterances - L rows, each call idling down to its longest group;
  * session:  open_session(max_live = L, max_samples = B), every utterance submitted with n_samples = B.
With the terminator muted every sample of a group reaches the length cap on the same step (the last is kept), so both arms generate
the same frames; admission_stream_ms_per_request then contains the K/V copies to the B - 1 sibling slots.
--stream: instead of the above, per size, every request streams (DecodeSession.submit(stream=True)):
  * streamer: voicecraft_amd.stream.SessionStreamer pumped until the session is idle - frames pulled while the batch decodes, ONE
    decode_streams feed per pump (--chunk-frames, default 8);
  * drain:    the same session with drain(), then one blocking tokenizer.decode per result.
One JSON line: per-request time to first audio (from the moment all requests were submitted; drain arm: to the end of that request's
decode) and the total time of both arms, interleaved pairs; both arms' audio lengths are asserted equal.  A second line measures the
codec alone: L streams of --codec-frames frames in chunks of --chunk-frames, all L in one decode_streams call per chunk against the
same L streams fed one call each.  Every special token is muted so that the generated ids are codec ids.
--cancel-share F (TTS only): instead of the above, per size, that fraction of the requests (evenly spread) are VICTIMS, in three legs on
one engine, interleaved (every request is submitted before the first turn):
  * run:    the victims run to their end - all a caller could do before DecodeSession.cancel existed;
  * cancel: the victims are cancelled --cancel-after turns after submission (live ones are retired by the next turn, pending ones leave
            the queue);
  * absent: the victims are never submitted - the bound.
One JSON line: the SURVIVORS' codec-tokens/s of each leg (the victims' frames are not counted in any), the per-pair position of the
cancel leg between the other two, how many victims were live and pending when cancelled, and the turns and milliseconds from the cancels
to the return of the turn that admits the next request (the one that takes a returned slot)."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from voicecraft_amd import synth
from voicecraft_amd.engine import VoiceCraftEngine

p = argparse.ArgumentParser()
p.add_argument("--preset", default="giga830M")
p.add_argument("--dtype", default="bf16")
p.add_argument("--lx", type=int, default=80)
p.add_argument("--lx-min", type=int, default=40)
p.add_argument("--prompt-frames", type=int, default=150)
p.add_argument("--top-k", type=int, default=40)
p.add_argument("--pairs", type=int, default=5)
p.add_argument("--sizes", default="64:8,256:64")
p.add_argument("--edit-share", type=float, default=0.0)
p.add_argument("--best-of", type=int, default=1)
p.add_argument("--stream", action="store_true")
p.add_argument("--chunk-frames", type=int, default=8)
p.add_argument("--codec-frames", type=int, default=200)
p.add_argument("--cancel-share", type=float, default=0.0)
p.add_argument("--cancel-after", type=int, default=4)
args = p.parse_args()
BO = args.best_of
assert BO >= 1 and (BO == 1 or (args.edit_share == 0 and not args.stream)), "--best-of goes with TTS requests only"
assert args.cancel_share == 0 or (BO == 1 and args.edit_share == 0 and not args.stream), "--cancel-share goes with plain TTS requests only"
dev = torch.device("cuda", 0)
a = synth.make_args(args.preset)
K = a.n_codebooks
# (with editing requests in the mix every special token is muted, not only the TTS terminator: an edit then ends at the length cap
# too - its terminator is eog - and both arms generate the same frames whatever their seeds)
sd = synth.make_state_dict(a, seed=0, perturb=False, mute_eos=True, fast=True, mute_special=args.edit_share > 0 or args.stream)
kn = dict(top_k=args.top_k, top_p=1.0, temperature=1.0, stop_repetition=3, silence_tokens=[1388, 1898, 131])
ekn = dict(top_k=0, top_p=0.8, temperature=1.0, stop_repetition=-1)      # the editing front-end's defaults
span = (args.prompt_frames // 3, 2 * (args.prompt_frames // 3))


def stats(v):
    v = sorted(v)
    return dict(median=round(statistics.median(v), 3), min=round(v[0], 3), max=round(v[-1], 3), n=len(v))


def width_for(n):
    w = 1
    while w < n:
        w *= 2
    return w


def simulate_blocking_rows(steps, G):
    """(live row-steps, launched rows, launched steps) of ONE blocking call whose sequences take `steps` samples each: the first sample is
    outside the loop; batch k of G steps runs at the width the re-pack rule gives from the live count at the end of batch k - 2."""
    B = len(steps)
    longest = max(steps) - 1
    live_rows = sum(s - 1 for s in steps)
    rows = n = 0
    w, k = B, 0
    while k * G < longest:
        if k >= 2:
            alive = sum(1 for s in steps if s - 1 > (k - 1) * G)
            if alive >= 1:
                w = min(w, width_for(alive))
        rows += w * G
        n += G
        k += 1
    return live_rows, rows, n


for size in args.sizes.split(","):
    N, L = (int(v) for v in size.split(":"))
    assert L % BO == 0, (L, BO)
    LU = L // BO                  # utterances that fit the slots together
    lxs = [args.lx if LU == 1 else args.lx_min + (args.lx - args.lx_min) * (u % LU) // (LU - 1) for u in range(N)]
    prompts = [synth.random_prompt(a, lxs[u], args.prompt_frames, seed=1 + u) for u in range(N)]
    is_edit = [int((u + 1) * args.edit_share) > int(u * args.edit_share) for u in range(N)]
    xs = [q[0][0].to(dev) for q in prompts]
    ys = [q[2][0].to(dev) for q in prompts]
    eng = VoiceCraftEngine(a, sd, device=dev, dtype=args.dtype, max_seqs=L, max_positions=max(1024, args.lx * 11 + 64))
    G = int(eng.options().split("g=")[1].split("|")[0].split(",")[0])

    def baseline(seed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frames, sim = [], [0, 0, 0]
        for g0 in range(0, N, LU):
            grp = list(range(g0, min(N, g0 + LU)))
            tts, edits = [u for u in grp if not is_edit[u]], [u for u in grp if is_edit[u]]
            f = {}
            if tts:
                outs = eng.inference_tts_multi([xs[u] for u in tts], [ys[u] for u in tts], _seed=seed + g0, batch_size=BO, **kn)
                f.update({u: int(gen.shape[2]) for u, (res, gen) in zip(tts, outs)})
            if edits:
                outs = eng.inference_multi([xs[u] for u in edits], [ys[u] for u in edits], [[span]] * len(edits), _seed=seed + g0,
                                           silence_tokens=kn["silence_tokens"], **ekn)
                f.update({u: int(res.shape[2]) - (args.prompt_frames - (span[1] - span[0])) for u, res in zip(edits, outs)})
            frames += [f[u] for u in grp]
            for part in (tts, edits):
                if part:
                    # (best-of-B: the kept sample takes f + K steps, a dropped one f + 1 - it is dropped on the deciding step)
                    for i, v in enumerate(simulate_blocking_rows([f[u] + (K if j == 0 else 1) for u in part for j in range(BO)], G)):
                        sim[i] += v
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        return dict(tok_s=sum(frames) * K / wall, wall_ms=wall * 1e3, frames=frames, live_rows=sim[0], launched_rows=sim[1], steps=sim[2])

    def session(seed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with eng.open_session(L, max_samples=BO, **kn) as sess:
            mi = torch.tensor([[span]], dtype=torch.int64)
            tickets = [sess.submit_edit(xs[u].reshape(1, -1), torch.tensor([lxs[u]]), ys[u].unsqueeze(0), mi, seed=seed + u, **ekn)
                       if is_edit[u] else
                       sess.submit(xs[u].reshape(1, -1), torch.tensor([lxs[u]]), ys[u].unsqueeze(0), seed=seed + u, n_samples=BO) for u in range(N)]
            done = {t: (res, gen) for t, res, gen in sess.drain()}
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            st = sess.stats(timing=True)
        frames = [int(done[t][0].shape[2]) - (args.prompt_frames - (span[1] - span[0])) if is_edit[u] else int(done[t][1].shape[2])
                  for u, t in enumerate(tickets)]
        return dict(tok_s=sum(frames) * K / wall, wall_ms=wall * 1e3, frames=frames, live_rows=st["live_rows"],
                    launched_rows=st["launched_rows"], steps=(st["turns"] - 1) * G, admitted=st["admitted"],
                    admitted_while_live=st["admitted_while_live"], widenings=st["widenings"], narrowings=st["narrowings"],
                    admission_us=st["admission_us"])

    def stream_leg():
        from voicecraft_amd.codec import AudioTokenizer
        from voicecraft_amd.stream import SessionStreamer
        tok = AudioTokenizer(synth.make_codec_state_dict(0), device=dev, max_seconds=(args.lx * 10 + 16) * 320 / 16000.0, max_batch=L)

        def submit_all(sess, seed, stream):
            return [sess.submit(xs[u].reshape(1, -1), torch.tensor([lxs[u]]), ys[u].unsqueeze(0), seed=seed + u, stream=stream) for u in range(N)]

        def streamer(seed):
            torch.cuda.synchronize()
            with eng.open_session(L, **kn) as sess:
                pump = SessionStreamer(sess, tok, chunk_frames=args.chunk_frames)
                tickets = submit_all(sess, seed, True)
                t0 = time.perf_counter()
                first, samples, done = {}, {t: 0 for t in tickets}, set()
                while not (sess.idle and len(done) == N):
                    for t, wav, d in pump.pump():
                        if wav.shape[2] and t not in first:
                            torch.cuda.current_stream(dev).synchronize()
                            first[t] = time.perf_counter() - t0
                        samples[t] += int(wav.shape[2])
                        if d:
                            done.add(t)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
            return dict(wall_ms=wall * 1e3, first_ms=[first[t] * 1e3 for t in tickets], samples=[samples[t] for t in tickets])

        def drained(seed):
            torch.cuda.synchronize()
            with eng.open_session(L, **kn) as sess:
                tickets = submit_all(sess, seed, False)
                t0 = time.perf_counter()
                res = {t: gen for t, _, gen in sess.drain()}
                first, samples = {}, {}
                for t in tickets:
                    wav = tok.decode([(res[t], None)])
                    torch.cuda.synchronize()
                    first[t] = time.perf_counter() - t0
                    samples[t] = int(wav.shape[2])
                wall = time.perf_counter() - t0
            return dict(wall_ms=wall * 1e3, first_ms=[first[t] * 1e3 for t in tickets], samples=[samples[t] for t in tickets])

        streamer(0); drained(0)
        rows = {"streamer": [], "drain": []}
        for i in range(args.pairs):
            for arm in (["streamer", "drain"] if i % 2 == 0 else ["drain", "streamer"]):
                rows[arm].append(streamer(100 + i) if arm == "streamer" else drained(100 + i))
        for b_, s_ in zip(rows["drain"], rows["streamer"]):
            assert b_["samples"] == s_["samples"], "both arms produce the same audio length per request"
        out = {"workload": f"stream leg: {args.preset} {args.dtype}, top_k={args.top_k}, {N} streaming requests through {L} slots, chunk_frames "
                           f"{args.chunk_frames}, {min(rows['drain'][0]['samples']) // 320}..{max(rows['drain'][0]['samples']) // 320} generated frames",
               "pairs": args.pairs, "graph_steps": G}
        for arm in ("streamer", "drain"):
            r = rows[arm]
            out[arm] = {"wall_ms": stats([v["wall_ms"] for v in r]),
                        "first_audio_ms_median_over_requests": stats([statistics.median(v["first_ms"]) for v in r]),
                        "first_audio_ms_first_request": stats([v["first_ms"][0] for v in r]),
                        "first_audio_ms_worst_request": stats([max(v["first_ms"]) for v in r])}
        out["streamer_vs_drain_wall_pct"] = stats([100.0 * (s_["wall_ms"] / b_["wall_ms"] - 1.0) for b_, s_ in zip(rows["drain"], rows["streamer"])])
        print(json.dumps(out), flush=True)
        # the codec alone: L streams in one call per chunk against one call per stream and chunk
        T, ch = args.codec_frames, args.chunk_frames
        clips = [torch.randint(0, 2048, (1, 4, T), device=dev) for _ in range(L)]

        def codec(together):
            st = tok.decode_streams(L)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for f0 in range(0, T, ch):
                last = tuple(range(L)) if f0 + ch >= T else ()
                if together:
                    st.feed({k: clips[k][:, :, f0: f0 + ch] for k in range(L)}, last=last)
                else:
                    for k in range(L):
                        st.feed({k: clips[k][:, :, f0: f0 + ch]}, last=(k,) if last else ())
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, st.census()
        codec(True); codec(False)
        ms = {True: [], False: []}
        for i in range(args.pairs):
            for arm in ((True, False) if i % 2 == 0 else (False, True)):
                ms[arm].append(codec(arm)[0])
        print(json.dumps({"workload": f"codec alone: {L} streams of {T} frames in chunks of {ch}", "pairs": args.pairs,
                          "one_call_per_chunk_ms": stats(ms[True]), "one_call_per_stream_and_chunk_ms": stats(ms[False]),
                          "census_of_a_joint_call": list(codec(True)[1]),
                          "joint_vs_separate_pct": stats([100.0 * (a_ / b_ - 1.0) for a_, b_ in zip(ms[True], ms[False])])}), flush=True)

    def cancel_legs():
        victim = [int((u + 1) * args.cancel_share) > int(u * args.cancel_share) for u in range(N)]

        def leg(mode, seed):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            was, wait, mark = {"pending": 0, "live": 0, "finished": 0}, None, None
            with eng.open_session(L, **kn) as sess:
                tickets = {u: sess.submit(xs[u].reshape(1, -1), torch.tensor([lxs[u]]), ys[u].unsqueeze(0), seed=seed + u)
                           for u in range(N) if not (mode == "absent" and victim[u])}
                done, turn = {}, 0
                while not sess.idle:
                    if mode == "cancel" and turn == args.cancel_after:
                        for u in range(N):
                            if victim[u]:
                                was[sess.cancel(tickets[u])] += 1
                        if was["live"]:
                            mark = (turn, time.perf_counter(), sess.stats()["admitted"])
                    for t, res, gen in sess.poll():
                        done[t] = int(gen.shape[2])
                    turn += 1
                    if mark is not None and sess.stats()["admitted"] > mark[2]:
                        # (turns: index of the admitting turn minus index of the first turn after the cancel - 2 by the release rule)
                        wait, mark = (turn - 1 - mark[0], (time.perf_counter() - mark[1]) * 1e3), None
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                st = sess.stats()
            frames = [done[tickets[u]] for u in range(N) if not victim[u]]
            return dict(tok_s=sum(frames) * K / wall, wall_ms=wall * 1e3, frames=frames, was=was, wait=wait, turns=st["turns"],
                        live_rows=st["live_rows"], launched_rows=st["launched_rows"])

        modes = ["run", "cancel", "absent"]
        for m in modes:
            leg(m, 0)
        rows = {m: [] for m in modes}
        for i in range(args.pairs):
            for m in modes[i % 3:] + modes[: i % 3]:
                rows[m].append(leg(m, 100 + i))
        for r_, c_, a_ in zip(rows["run"], rows["cancel"], rows["absent"]):
            assert r_["frames"] == c_["frames"] == a_["frames"], "the survivors generate the same frames in every leg (the length cap ends them)"
        c0 = rows["cancel"][0]
        out = {"workload": f"cancel legs: {args.preset} {args.dtype}, top_k={args.top_k}, {N} requests through {L} slots, {sum(victim)} of them "
                           f"victims cancelled {args.cancel_after} turns after submission, survivors of {min(c0['frames'])}..{max(c0['frames'])} frames",
               "pairs": args.pairs, "graph_steps": G, "victims_were": c0["was"]}
        for m in modes:
            out[m] = {"survivor_codec_tokens_per_s": stats([v["tok_s"] for v in rows[m]]), "wall_ms": stats([v["wall_ms"] for v in rows[m]]),
                      "turns": rows[m][0]["turns"], "live_share_of_launched_rows": round(rows[m][0]["live_rows"] / rows[m][0]["launched_rows"], 4)}
        # 0 = no better than letting the victims run, 1 = as good as never having had them
        out["cancel_position_between_run_and_absent"] = stats([(c_["tok_s"] - r_["tok_s"]) / (a_["tok_s"] - r_["tok_s"])
                                                               for r_, c_, a_ in zip(rows["run"], rows["cancel"], rows["absent"])])
        waits = [v["wait"] for v in rows["cancel"] if v["wait"] is not None]
        if waits:
            out["cancel_to_next_admission"] = {"turns": stats([w[0] for w in waits]), "ms": stats([w[1] for w in waits])}
        print(json.dumps(out), flush=True)

    if args.stream or args.cancel_share > 0:
        stream_leg() if args.stream else cancel_legs()
        del eng
        torch.cuda.empty_cache()
        continue
    baseline(0); session(0)                    # graphs captured, allocator warm
    rows = {"baseline": [], "session": []}
    for i in range(args.pairs):
        order = ["baseline", "session"] if i % 2 == 0 else ["session", "baseline"]
        for arm in order:
            rows[arm].append(baseline(100 + i) if arm == "baseline" else session(100 + i))
    for b, s in zip(rows["baseline"], rows["session"]):
        assert b["frames"] == s["frames"], "both arms generate the same frames per utterance (the length cap ends every sequence)"
    out = {"workload": f"{args.preset} {args.dtype}, top_k={args.top_k}, {N} utterances ({sum(is_edit)} of them editing requests) through {L} slots, Lx {min(lxs)}..{max(lxs)}, "
                       f"{args.prompt_frames} prompt frames -> {min(rows['session'][0]['frames'])}..{max(rows['session'][0]['frames'])} generated frames",
           "pairs": args.pairs, "graph_steps": G, "best_of": BO, "options": eng.options()}
    for arm in ("baseline", "session"):
        r = rows[arm]
        out[arm] = {"codec_tokens_per_s": stats([v["tok_s"] for v in r]), "wall_ms": stats([v["wall_ms"] for v in r]),
                    "mean_live_rows_per_launched_step": round(statistics.mean(v["live_rows"] / v["steps"] for v in r), 2),
                    "live_share_of_launched_rows": round(statistics.mean(v["live_rows"] / v["launched_rows"] for v in r), 4),
                    "launched_steps": r[0]["steps"]}
    s0 = rows["session"]
    out["session"].update({k: s0[0][k] for k in ("admitted", "admitted_while_live", "widenings", "narrowings")})
    out["session"]["admission_stream_ms_per_request"] = stats([v["admission_us"] / 1e3 / v["admitted"] for v in s0])
    out["session_vs_baseline_pct"] = stats([100.0 * (s["tok_s"] / b["tok_s"] - 1.0) for b, s in zip(rows["baseline"], rows["session"])])
    print(json.dumps(out), flush=True)
    del eng
    torch.cuda.empty_cache()
