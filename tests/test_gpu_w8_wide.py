"""-m gpu: option `w8w` - on an engine created with `w8=` and `w8_wide=True`, steps of 17..64 rows stream the FFN down-projection
(bit 1) and the QKV projection of every layer (bit 4) as E4M3 pair planes of their 16-channel images (rows_gemm_wds_w8_k).  The bytes
decode to the same bf16 MFMA operands and everything else is the staged wide kernel's text (csrc/vc_gemm_wds_body.h), so every result
is BIT-identical to `w8w = 0`: the tests compare with np.array_equal only, eager and captured, at every width with a form (tiny128: 2
k-tiles per wave; giga330M: 4; giga830M: 8), at both row-tile counts and their edges (17 = a second row tile with one row, 32 / 33 = two
-> four row tiles, 48 = a fourth tile without rows, 64), with inactive rows and narrowing steps, a refused matrix, the 8-bit K/V cache
and a decode session.  Bit 8 of the option takes the form whatever the measured win table says, so the kernel is always reached."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_STEPS = 12
LAYERS = 2
OFF_GRID = (1.0 + 2.0 ** -7) * 2.0 ** -6          # eight significant bits: on no E4M3 grid (tests/test_gpu_w8.py)
CASES = [("tiny128", r) for r in (17, 32, 33, 48, 64)] + [(p, r) for p in ("giga330M", "giga830M") for r in (17, 33, 64)]
WD_PER_STEP = 4 * LAYERS + 2                      # rows_gemm_wd_k launches of a wide step: four per layer, two for the heads


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


@functools.lru_cache(maxsize=None)
def _model(preset, live=False):
    """(args, the synthetic state dict on the w8 grid, 64 prompts of different shapes): computed once, never modified.
    live: terminators can be sampled (the recipe of tests/test_gpu_session.py), so that free-running calls end by themselves."""
    from voicecraft_amd import quant, synth
    a = synth.make_args(preset, num_decoder_layers=LAYERS)
    sd = synth.make_state_dict(a, seed=4, fast=True, mute_eos=False, boost=[(0, 2051, 0.45)]) if live else synth.make_state_dict(a, seed=0, fast=True)
    prompts = tuple(synth.random_prompt(a, 4 + (u % 5), 9 + 3 * (u % 7), seed=700 + u) for u in range(64))
    return a, quant.quantize_state_dict_w8(a, sd), prompts


def _forced(a, rows, ends=None):
    """[N_STEPS][rows][K] forced tokens; row u ends with step ends[u] (default: the last), by the staggered end of a span
    (voicecraft.py:1057-1066): the call ends with its forced steps."""
    K = a.n_codebooks
    toks = np.random.RandomState(17).randint(0, a.audio_vocab_size, size=(N_STEPS, rows, K)).astype(np.int64)
    for u in range(rows):
        n = N_STEPS if ends is None else ends[u]
        for j in range(K):
            toks[n - K + j, u, :j] = a.empty_token
            toks[n - K + j, u, j] = a.eos
    return toks


def _engine(a, sd, rows, w8="as_is", w8_wide=True, use_graph=True, cls=None, **kw):
    from voicecraft_amd.engine import VoiceCraftEngine
    if w8 is not None:
        kw["w8"] = w8
    return (cls or VoiceCraftEngine)(a, sd, device="cuda:0", dtype="bf16", max_seqs=rows, max_positions=256, use_graph=use_graph,
                                     w8_wide=w8_wide, **kw)


def _multi(eng, prompts, rows, forced):
    outs, lg = eng.inference_tts_multi([p[0][0] for p in prompts[:rows]], [p[2][0] for p in prompts[:rows]], top_k=1, stop_repetition=3,
                                       _forced=forced, _logit_steps=N_STEPS)
    return [o[0].cpu().numpy() for o in outs], lg.cpu().numpy()


def _plan(eng, a, mask, rows):
    """vc_debug_w8w_plan for the engine's model shape: (FFN-down, QKV) take the form"""
    from test_w8_rows_cpu import cfg
    out = (C.c_int32 * 4)()
    c = cfg(a.d_model, a.nhead)
    assert eng.lib.vc_debug_w8w_plan(C.byref(c), mask, rows, out) == 0
    return out[0], out[1]


@pytest.mark.parametrize("preset,rows", CASES)
def test_w8w_logits_bit_identical_and_census(preset, rows):
    a, sdq, prompts = _model(preset)
    forced = _forced(a, rows)
    eng = _engine(a, sdq, rows)
    assert eng.options().endswith("|w8=5|w8w=5")
    st = eng.w8_stats()
    assert all(layer["ffn_down_wide"] == {"state": "packed", "refused_pairs": 0} and layer["qkv_wide"] == {"state": "packed", "refused_pairs": 0}
               for layer in st), st
    assert _plan(eng, a, 13, rows) == (1, 1)
    for use_graph in (False, True):
        eng.use_graph = use_graph
        ref = None
        for v in (0, 9, 12, 13):
            eng.set_option("w8w", v)
            assert eng.options().endswith(f"|w8=5|w8w={v}")
            c0 = eng.launch_counts()
            res, lg = _multi(eng, prompts, rows, forced)
            c = _delta(eng.launch_counts(), c0)
            assert eng.last_steps == N_STEPS             # every row ends with the last forced step: the step width never changes
            if ref is None:
                ref = (res, lg, c)
                assert np.isfinite(lg[np.abs(lg) < 1e3]).all() and np.abs(lg).max() > 0
                assert c["w8_wide"] == 0, c
            assert np.array_equal(lg, ref[1]), (use_graph, v, float(np.abs(lg - ref[1]).max()))
            assert all(np.array_equal(r, w) for r, w in zip(res, ref[0]))
            # one FFN down-projection and one QKV projection per layer and step (eager: every launch is counted, captured: once per
            # capture), each counted in rows_gemm_wd_k's slot and once more in w8_wide
            assert c["wd"] > 0 and c["wd"] % WD_PER_STEP == 0, c
            steps = c["wd"] // WD_PER_STEP
            if not use_graph:                            # (the eager loop launches steps ahead of the ones it takes)
                assert steps >= N_STEPS - 1, c
            assert c["w8_wide"] == steps * LAYERS * ((v & 1) + (v & 4) // 4), (use_graph, v, c)
            # the option moves no launch to another form.  (Captured: every launch is counted once, at capture.  The eager loop launches
            # steps ahead of the ones it takes, a number that depends on the host's timing: there only the fixed slots are compared.)
            for slot in c:
                if slot != "w8_wide" and (use_graph or slot in ("w8", "w13", "w8_rows", "row_gemm_fr1", "rows_gemm_frp", "rows_gemm_qp")):
                    assert c[slot] == ref[2][slot], (slot, v, c, ref[2])


def test_w8w_without_bit_8_follows_the_plan():
    a, sdq, prompts = _model("giga830M")
    rows = 33
    forced = _forced(a, rows)
    eng = _engine(a, sdq, rows, use_graph=False)
    eng.set_option("w8w", 0)
    _, want = _multi(eng, prompts, rows, forced)
    eng.set_option("w8w", 5)
    assert eng.options().endswith("|w8=5|w8w=5")
    ffn, qkv = _plan(eng, a, 5, rows)
    c0 = eng.launch_counts()
    _, got = _multi(eng, prompts, rows, forced)
    c = _delta(eng.launch_counts(), c0)
    assert c["wd"] % WD_PER_STEP == 0 and c["w8_wide"] == c["wd"] // WD_PER_STEP * LAYERS * (ffn + qkv), (c, ffn, qkv)
    assert np.array_equal(got, want)


# (rows, rows that end six steps early, live rows afterwards, w8_rows)
SCHEDULES = [(33, [0] + list(range(20, 33)), 19, False),        # shrink: 33 -> 32 rows, four row tiles -> two
             (17, [0], 16, False),                              # shrink: 17 -> 16 rows, the engine leaves the wide form
             (17, list(range(8, 17)), 8, True)]                 # shrink: 17 -> 8 rows, the tail on the w8r forms


@pytest.mark.parametrize("shrink", [1, 0])
@pytest.mark.parametrize("rows,early,live,w8_rows", SCHEDULES)
def test_w8w_inactive_and_ragged_rows(rows, early, live, w8_rows, shrink):
    """Some rows end six steps before the others: with shrink off they stay in the step without a position, with shrink on the live
    rows move onto a narrower step."""
    a, sdq, prompts = _model("giga830M")
    forced = _forced(a, rows, ends=[N_STEPS - 6 if u in early else N_STEPS for u in range(rows)])
    eng = _engine(a, sdq, rows, w8_rows=w8_rows)
    eng.set_option("shrink", shrink)
    out = {}
    for v in (0, 13):
        eng.set_option("w8w", v)
        c0 = eng.launch_counts()
        out[v] = _multi(eng, prompts, rows, forced)
        c = _delta(eng.launch_counts(), c0)
        assert (c["w8_wide"] > 0) == bool(v), c
        if w8_rows and shrink:                                  # the 8-row tail of the narrowed call runs rows_gemm_frp_w8_k
            assert c["w8_rows"] >= LAYERS and c["rows_gemm_frp"] >= LAYERS, c
    (res0, lg0), (res1, lg1) = out[0], out[13]
    T = [p[2].shape[1] for p in prompts[:rows]]
    late = next(u for u in range(rows) if u not in early)
    assert res0[early[0]].shape[-1] - T[early[0]] < res0[late].shape[-1] - T[late], [r.shape for r in res0]
    assert all(r0.shape == r1.shape and np.array_equal(r0, r1) for r0, r1 in zip(res0, res1))
    assert np.array_equal(lg0, lg1), float(np.abs(lg0 - lg1).max())


def test_w8w_one_off_grid_value_keeps_its_layer_on_the_image():
    a, sdq, prompts = _model("giga330M")
    sdq = {k: v.clone() for k, v in sdq.items()}
    sdq["decoder.layers.1.linear2.weight"][9, 200] = OFF_GRID
    rows = 33
    forced = _forced(a, rows)
    eng = _engine(a, sdq, rows, use_graph=False)
    st = eng.w8_stats()
    assert st[0]["ffn_down_wide"] == {"state": "packed", "refused_pairs": 0}, st
    assert st[1]["ffn_down_wide"] == {"state": "refused", "refused_pairs": 1}, st
    assert all(layer["qkv_wide"]["state"] == "packed" for layer in st), st
    _, want = _multi(_engine(a, sdq, rows, w8=None, w8_wide=False, use_graph=False), prompts, rows, forced)
    # eager: every launch is counted; layer 1's FFN down-projection stays on rows_gemm_wds_k
    for v, per_step in ((9, LAYERS - 1), (12, LAYERS), (13, 2 * LAYERS - 1)):
        eng.set_option("w8w", v)
        c0 = eng.launch_counts()
        _, got = _multi(eng, prompts, rows, forced)
        c = _delta(eng.launch_counts(), c0)
        steps = c["wd"] // WD_PER_STEP
        assert steps >= N_STEPS - 1 and c["wd"] == steps * WD_PER_STEP, c
        assert c["w8_wide"] == steps * per_step, (v, c)
        assert np.array_equal(got, want), v


def test_w8w_with_the_8_bit_kv_cache():
    """kv8 changes values, identically in both legs: 64 rows at giga830M, w8w 13 against 0."""
    a, sdq, prompts = _model("giga830M")
    rows = 64
    forced = _forced(a, rows)
    eng = _engine(a, sdq, rows, kv8=True)
    assert eng.options().endswith("|w8=5|w8w=5|kv8=1")
    out = {}
    for v in (0, 13):
        eng.set_option("w8w", v)
        c0 = eng.launch_counts()
        out[v] = _multi(eng, prompts, rows, forced)
        c = _delta(eng.launch_counts(), c0)
        assert (c["w8_wide"] > 0) == bool(v) and c["kv8_attn"] > 0, c
    assert all(np.array_equal(r0, r1) for r0, r1 in zip(out[0][0], out[13][0]))
    assert np.array_equal(out[0][1], out[13][1])


def test_w8w_decode_session_twenty_slots():
    """24 seeded requests of different lengths through 20 slots: the step is wide while more than 16 slots are live."""
    a, sdq, prompts = _model("giga830M", live=True)
    got = {}
    for v in (0, 13):
        eng = _engine(a, sdq, 20)
        eng.set_option("w8w", v)
        c0 = eng.launch_counts()
        outs = eng.inference_tts_queue([p[0][0] for p in prompts[:24]], [p[2][0] for p in prompts[:24]], max_live=20,
                                       seeds=[100 + u for u in range(24)], top_k=40, top_p=1.0, temperature=1.0, stop_repetition=3)
        c = _delta(eng.launch_counts(), c0)
        assert eng.last_session_stats["admitted"] == 24, eng.last_session_stats
        assert c["wd"] > 0 and (c["w8_wide"] > 0) == bool(v), c
        got[v] = [o[0].cpu().numpy() for o in outs]
        del eng
    assert all(r0.shape == r1.shape and np.array_equal(r0, r1) for r0, r1 in zip(got[0], got[13]))


def test_no_request_nothing_new():
    from test_w8_rows_cpu import cfg
    from voicecraft_amd.engine import VoiceCraftEngine
    a, sdq, prompts = _model("tiny128")
    rows = 33
    forced = _forced(a, rows)
    eng = _engine(a, sdq, rows, w8="quantize", w8_wide=False)
    assert eng.options().endswith("|w13=5|w8=5") and "w8w" not in eng.options()
    assert all("ffn_down_wide" not in layer and "qkv_wide" not in layer for layer in eng.w8_stats())
    for v in (0, 1, 5, 13):
        with pytest.raises(AssertionError):
            eng.set_option("w8w", v)
        assert eng.options().endswith("|w13=5|w8=5")
    c0 = eng.launch_counts()
    _multi(eng, prompts, rows, forced)
    c = _delta(eng.launch_counts(), c0)
    assert c["w8_wide"] == 0 and c["wd"] > 0, c
    assert eng.lib.vc_request_w8_wide(eng._h, 5) == -2          # VC_ESTATE: the request comes before vc_finalize_weights
    with pytest.raises(ValueError):
        _engine(a, sdq, rows, w8=None, w8_wide=True)
    for bad in (2, 7, 8, 13, -1):                                # not a mask of 1 | 4: VC_EINVAL, an AssertionError as for every bad input
        bad_cls = type("BadMask", (VoiceCraftEngine,), {"W8_WIDE_MASK": bad})
        with pytest.raises(AssertionError):
            _engine(a, sdq, rows, cls=bad_cls)
    no_subset = type("NoSubset", (VoiceCraftEngine,), {"W8_MASK": 1})      # the wide mask must be a subset of vc_request_w8's
    with pytest.raises(AssertionError):
        _engine(a, sdq, rows, cls=no_subset)
    # the order of the requests, on a bare handle
    lib = eng.lib
    h = C.c_void_p()
    c = cfg(a.d_model, a.nhead)
    assert lib.vc_create(C.byref(c), 0, C.byref(h)) == 0
    try:
        assert lib.vc_request_w8_wide(h, 5) == -2               # VC_ESTATE: after vc_request_w8 only
        assert lib.vc_request_w8(h, 1) == 0
        assert lib.vc_request_w8_wide(h, 4) == -1               # VC_EINVAL: no subset of the w8 request
        assert lib.vc_request_w8_wide(h, 5) == -1
        assert lib.vc_request_w8_wide(h, 2) == -1
        assert lib.vc_request_w8_wide(h, 1) == 0
    finally:
        lib.vc_destroy(h)
    eng8 = _engine(a, sdq, rows)
    for bad in (2, 7, 16, 21, -1):
        with pytest.raises(AssertionError):
            eng8.set_option("w8w", bad)
        assert eng8.options().endswith("|w8=5|w8w=5")
    # an engine that cannot run wide steps packs nothing more and plans nothing
    narrow = _engine(a, sdq, 8)
    assert all(layer["ffn_down_wide"]["state"] == "not_applicable" and layer["qkv_wide"]["state"] == "not_applicable"
               for layer in narrow.w8_stats()), narrow.w8_stats()
