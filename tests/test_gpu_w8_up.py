"""-m gpu: option `w8u` - on an engine created with `w8=` and `w8_up=True`, steps of 17..64 rows stream the FFN up-projection of every
layer (bit 2) as E4M3 pair planes of its 16-channel image (rows_gemm_wds_w8u_k).  The bytes decode to the same bf16 MFMA operands and
everything else is the staged wide kernel's text (csrc/vc_gemm_wds_body.h) with the image launch's epilogue, so every result is
BIT-identical to `w8u = 0`: the tests compare with np.array_equal only, eager and captured, at every width with a form (tiny128: 2
k-tiles per wave; giga330M: 4; giga830M: 8), at both row-tile counts and their edges (17 = a second row tile with one row, 32 / 33 = two
-> four row tiles, 48 = a fourth tile without rows, 64), next to `w8w`, with inactive rows and narrowing steps, a refused layer, the
8-bit K/V cache and a decode session.  Value 10 (bit 8) takes the form whatever the measured win table says, so the kernel is always
reached.  The one tolerance is the project's bf16 bar against the oracle on the three-matrix checkpoint."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_STEPS = 12
LAYERS = 2
OFF_GRID = (1.0 + 2.0 ** -7) * 2.0 ** -6          # eight significant bits: on no E4M3 grid (tests/test_gpu_w8.py)
CASES = [("tiny128", r) for r in (17, 32, 33, 48, 64)] + [(p, r) for p in ("giga330M", "giga830M") for r in (17, 33, 64)]
KPW = {"tiny128": 2, "giga330M": 4, "giga830M": 8}
WD_PER_STEP = 4 * LAYERS + 2                      # rows_gemm_wd_k launches of a wide step: four per layer, two for the heads
PACKED = {"state": "packed", "refused_pairs": 0}
# slots the eager loop (which launches steps ahead of the ones it takes, a number that depends on the host's timing) cannot move
FIXED_SLOTS = ("w8", "w13", "w8_rows", "w8_mid", "row_gemm_fr1", "rows_gemm_frp", "rows_gemm_qp")


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


@functools.lru_cache(maxsize=None)
def _model(preset, live=False):
    """(args, the synthetic state dict with THREE matrices on the w8 grid, 64 prompts of different shapes): computed once, never
    modified.  live: terminators can be sampled (the recipe of tests/test_gpu_session.py), so that free-running calls end by themselves."""
    from voicecraft_amd import quant, synth
    a = synth.make_args(preset, num_decoder_layers=LAYERS)
    sd = synth.make_state_dict(a, seed=4, fast=True, mute_eos=False, boost=[(0, 2051, 0.45)]) if live else synth.make_state_dict(a, seed=0, fast=True)
    prompts = tuple(synth.random_prompt(a, 4 + (u % 5), 9 + 3 * (u % 7), seed=700 + u) for u in range(64))
    return a, quant.quantize_state_dict_w8(a, sd, ffn_up=True), prompts


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


def _engine(a, sd, rows, w8="as_is", w8_up=True, use_graph=True, cls=None, dtype="bf16", **kw):
    from voicecraft_amd.engine import VoiceCraftEngine
    if w8 is not None:
        kw["w8"] = w8
    return (cls or VoiceCraftEngine)(a, sd, device="cuda:0", dtype=dtype, max_seqs=rows, max_positions=256, use_graph=use_graph,
                                     w8_up=w8_up, **kw)


def _multi(eng, prompts, rows, forced):
    outs, lg = eng.inference_tts_multi([p[0][0] for p in prompts[:rows]], [p[2][0] for p in prompts[:rows]], top_k=1, stop_repetition=3,
                                       _forced=forced, _logit_steps=N_STEPS)
    return [o[0].cpu().numpy() for o in outs], lg.cpu().numpy()


def _plan(eng, a, mask, rows):
    """vc_debug_w8u_plan for the engine's model shape: (the form is taken, k-tiles per wave)"""
    from test_w8_rows_cpu import cfg
    out = (C.c_int32 * 2)()
    c = cfg(a.d_model, a.nhead)
    assert eng.lib.vc_debug_w8u_plan(C.byref(c), mask, rows, out) == 0
    return out[0], out[1]


@pytest.mark.parametrize("preset,rows", CASES)
def test_w8u_logits_bit_identical_and_census(preset, rows):
    a, sdq, prompts = _model(preset)
    forced = _forced(a, rows)
    eng = _engine(a, sdq, rows)
    assert eng.options().endswith("|w8=5|w8u=2")
    st = eng.w8_stats()
    assert all(layer["ffn_up_wide"] == PACKED and "ffn_down_wide" not in layer and "qkv_wide" not in layer for layer in st), st
    assert _plan(eng, a, 10, rows) == (1, KPW[preset])
    for use_graph in (False, True):
        eng.use_graph = use_graph
        ref = None
        for v in (0, 2, 10):
            eng.set_option("w8u", v)
            assert eng.options().endswith(f"|w8=5|w8u={v}")
            c0 = eng.launch_counts()
            res, lg = _multi(eng, prompts, rows, forced)
            c = _delta(eng.launch_counts(), c0)
            assert eng.last_steps == N_STEPS             # every row ends with the last forced step: the step width never changes
            if ref is None:
                ref = (res, lg, c)
                assert np.isfinite(lg[np.abs(lg) < 1e3]).all() and np.abs(lg).max() > 0
                assert c["w8_up"] == 0, c
            assert np.array_equal(lg, ref[1]), (use_graph, v, float(np.abs(lg - ref[1]).max()))
            assert all(np.array_equal(r, w) for r, w in zip(res, ref[0]))
            # one FFN up-projection per layer and step (eager: every launch is counted, captured: once per capture), counted in
            # rows_gemm_wd_k's slot and once more in w8_up - where the plan takes the form (value 2: the measured table decides)
            assert c["wd"] > 0 and c["wd"] % WD_PER_STEP == 0, c
            steps = c["wd"] // WD_PER_STEP
            if not use_graph:                            # (the eager loop launches steps ahead of the ones it takes)
                assert steps >= N_STEPS - 1, c
            assert c["w8_up"] == steps * LAYERS * _plan(eng, a, v, rows)[0], (use_graph, v, c)
            if v == 10:
                assert c["w8_up"] == steps * LAYERS
            # the option moves no launch to another form and counts in no older slot
            for slot in c:
                if slot != "w8_up" and (use_graph or slot in FIXED_SLOTS + ("w8_wide",)):
                    assert c[slot] == ref[2][slot], (slot, v, c, ref[2])
            assert c["w8_wide"] == 0, c


def test_w8u_next_to_the_wide_form():
    """`w8w` 13 and `w8u` 10 on one engine against both off: three matrices of the layer on pair planes; w8_wide keeps its formula."""
    a, sdq, prompts = _model("giga830M")
    rows = 33
    forced = _forced(a, rows)
    eng = _engine(a, sdq, rows, w8_wide=True, use_graph=False)
    assert eng.options().endswith("|w8=5|w8w=5|w8u=2")
    st = eng.w8_stats()
    assert all(layer["ffn_up_wide"] == PACKED and layer["ffn_down_wide"] == PACKED and layer["qkv_wide"] == PACKED for layer in st), st
    out = {}
    for w, u in ((0, 0), (13, 10), (13, 0), (0, 10)):
        eng.set_option("w8w", w)
        eng.set_option("w8u", u)
        assert eng.options().endswith(f"|w8=5|w8w={w}|w8u={u}")
        c0 = eng.launch_counts()
        out[w, u] = _multi(eng, prompts, rows, forced)
        c = _delta(eng.launch_counts(), c0)
        steps = c["wd"] // WD_PER_STEP
        assert steps >= N_STEPS - 1 and c["wd"] == steps * WD_PER_STEP, c
        assert c["w8_wide"] == steps * LAYERS * ((w & 1) + (w & 4) // 4), (w, u, c)
        assert c["w8_up"] == steps * LAYERS * (u & 2) // 2, (w, u, c)
    for key in out:
        assert all(np.array_equal(r0, r1) for r0, r1 in zip(out[0, 0][0], out[key][0])), key
        assert np.array_equal(out[0, 0][1], out[key][1]), key


def test_as_is_without_the_request_computes_the_same_checkpoint():
    """The three-matrix checkpoint is an ordinary state dict: an engine without `w8_up` (and one without `w8=`) gives the same logits."""
    a, sdq, prompts = _model("tiny128")
    rows = 33
    forced = _forced(a, rows)
    eng = _engine(a, sdq, rows)
    eng.set_option("w8u", 10)
    c0 = eng.launch_counts()
    res, lg = _multi(eng, prompts, rows, forced)
    assert _delta(eng.launch_counts(), c0)["w8_up"] > 0
    for kw in (dict(w8="as_is", w8_up=False), dict(w8=None, w8_up=False)):
        other = _engine(a, sdq, rows, **kw)
        assert "w8u" not in other.options() and all("ffn_up_wide" not in layer for layer in other.w8_stats())
        c0 = other.launch_counts()
        res1, lg1 = _multi(other, prompts, rows, forced)
        assert _delta(other.launch_counts(), c0)["w8_up"] == 0
        assert np.array_equal(lg, lg1) and all(np.array_equal(r0, r1) for r0, r1 in zip(res, res1)), kw


# (rows, rows that end six steps early, live rows afterwards)
SCHEDULES = [(33, [0] + list(range(20, 33)), 19),        # shrink: 33 -> 32 rows, four row tiles -> two
             (17, [0], 16)]                              # shrink: 17 -> 16 rows, the engine leaves the wide form


@pytest.mark.parametrize("shrink", [1, 0])
@pytest.mark.parametrize("rows,early,live", SCHEDULES)
def test_w8u_inactive_and_ragged_rows(rows, early, live, shrink):
    """Some rows end six steps before the others: with shrink off they stay in the step without a position, with shrink on the live
    rows move onto a narrower step; up to 16 rows that step reads the bf16 image of the same values and `w8_up` stops counting."""
    a, sdq, prompts = _model("giga830M")
    forced = _forced(a, rows, ends=[N_STEPS - 6 if u in early else N_STEPS for u in range(rows)])
    eng = _engine(a, sdq, rows)
    eng.set_option("shrink", shrink)
    out = {}
    for v in (0, 10):
        eng.set_option("w8u", v)
        c0 = eng.launch_counts()
        out[v] = _multi(eng, prompts, rows, forced)
        c = _delta(eng.launch_counts(), c0)
        # exactly the wide steps count (captured: once per capture, as their rows_gemm_wd_k launches)
        assert c["wd"] > 0 and c["wd"] % WD_PER_STEP == 0, c
        assert c["w8_up"] == (c["wd"] // WD_PER_STEP * LAYERS if v else 0), (v, c)
        if shrink and rows == 17:                               # the 16-row tail runs the finished-row forms
            assert c["rows_gemm_fr"] > 0, c
    (res0, lg0), (res1, lg1) = out[0], out[10]
    T = [p[2].shape[1] for p in prompts[:rows]]
    late = next(u for u in range(rows) if u not in early)
    assert res0[early[0]].shape[-1] - T[early[0]] < res0[late].shape[-1] - T[late], [r.shape for r in res0]
    assert all(r0.shape == r1.shape and np.array_equal(r0, r1) for r0, r1 in zip(res0, res1))
    assert np.array_equal(lg0, lg1), float(np.abs(lg0 - lg1).max())


def test_w8u_one_off_grid_value_keeps_its_layer_on_the_image():
    from voicecraft_amd import quant
    a, sdq, prompts = _model("giga330M")
    sdq = {k: v.clone() for k, v in sdq.items()}
    sdq["decoder.layers.1.linear1.weight"][9, 200] = OFF_GRID
    img = quant.fold(sdq["decoder.layers.1.linear1.weight"], sdq["decoder.layers.1.norm2.weight"])
    assert quant.quantize_image(img)[9, 200] != img[9, 200]             # the folded value is off the grid too
    rows = 33
    forced = _forced(a, rows)
    eng = _engine(a, sdq, rows, use_graph=False)
    st = eng.w8_stats()
    assert st[0]["ffn_up_wide"] == PACKED, st
    assert st[1]["ffn_up_wide"]["state"] == "refused" and st[1]["ffn_up_wide"]["refused_pairs"] >= 1, st
    eng.set_option("w8u", 0)
    res0, want = _multi(eng, prompts, rows, forced)
    # eager: every launch is counted; layer 1's FFN up-projection stays on rows_gemm_wds_k
    eng.set_option("w8u", 10)
    c0 = eng.launch_counts()
    res1, got = _multi(eng, prompts, rows, forced)
    c = _delta(eng.launch_counts(), c0)
    steps = c["wd"] // WD_PER_STEP
    assert steps >= N_STEPS - 1 and c["wd"] == steps * WD_PER_STEP, c
    assert c["w8_up"] == steps * (LAYERS - 1), c
    assert np.array_equal(got, want) and all(np.array_equal(r0, r1) for r0, r1 in zip(res0, res1))


def test_w8u_with_the_8_bit_kv_cache():
    """kv8 changes values, identically in both legs: 64 rows at giga830M, w8u 10 against 0."""
    a, sdq, prompts = _model("giga830M")
    rows = 64
    forced = _forced(a, rows)
    eng = _engine(a, sdq, rows, kv8=True)
    assert eng.options().endswith("|w8=5|w8u=2|kv8=1")
    out = {}
    for v in (0, 10):
        eng.set_option("w8u", v)
        c0 = eng.launch_counts()
        out[v] = _multi(eng, prompts, rows, forced)
        c = _delta(eng.launch_counts(), c0)
        assert (c["w8_up"] > 0) == bool(v) and c["kv8_attn"] > 0, c
    assert all(np.array_equal(r0, r1) for r0, r1 in zip(out[0][0], out[10][0]))
    assert np.array_equal(out[0][1], out[10][1])


def test_w8u_decode_session_twenty_slots():
    """24 seeded requests of different lengths through 20 slots: the step is wide while more than 16 slots are live."""
    a, sdq, prompts = _model("giga830M", live=True)
    got = {}
    for v in (0, 10):
        eng = _engine(a, sdq, 20)
        eng.set_option("w8u", v)
        c0 = eng.launch_counts()
        outs = eng.inference_tts_queue([p[0][0] for p in prompts[:24]], [p[2][0] for p in prompts[:24]], max_live=20,
                                       seeds=[100 + u for u in range(24)], top_k=40, top_p=1.0, temperature=1.0, stop_repetition=3)
        c = _delta(eng.launch_counts(), c0)
        assert eng.last_session_stats["admitted"] == 24, eng.last_session_stats
        assert c["wd"] > 0 and (c["w8_up"] > 0) == bool(v), c
        got[v] = [o[0].cpu().numpy() for o in outs]
        del eng
    assert all(r0.shape == r1.shape and np.array_equal(r0, r1) for r0, r1 in zip(got[0], got[10]))


def test_w8u_against_the_oracle_on_the_quantised_checkpoint():
    """`w8="quantize"` with `w8_up=True` quantises the third matrix too; teacher-forced logits of a 33-row call meet the project's
    bf16 bar (per-step relative L2 <= 2e-2) against the oracle on that checkpoint for three of the rows."""
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from test_gpu_model import rel_l2
    from voicecraft_amd import synth
    a, sdq, prompts = _model("tiny128")
    sd = synth.make_state_dict(a, seed=0, fast=True)
    rows = 33
    forced = _forced(a, rows)
    eng = _engine(a, sd, rows, w8="quantize")
    assert all(torch.equal(eng.w8_state_dict[k], sdq[k]) for k in sdq if torch.is_tensor(sdq[k]))
    assert not torch.equal(eng.w8_state_dict["decoder.layers.0.linear1.weight"], sd["decoder.layers.0.linear1.weight"])
    assert all(layer["ffn_up_wide"] == PACKED for layer in eng.w8_stats())
    eng.set_option("w8u", 10)
    c0 = eng.launch_counts()
    _, got = _multi(eng, prompts, rows, forced)
    assert _delta(eng.launch_counts(), c0)["w8_up"] > 0
    torch.set_num_threads(min(4, torch.get_num_threads()))
    orc = VoiceCraftOracle(a, eng.w8_state_dict)
    for u in (0, 16, 32):
        x, _, y = prompts[u]
        want = orc.tts_logits_for_trajectory(x, y, forced[:, u], steps=list(range(N_STEPS))).numpy()
        rel = float(rel_l2(got[:, u].reshape(want.shape), want).max())
        print(f"tiny128, 33 rows, utterance {u}: w8u engine against the oracle on the three-matrix checkpoint: worst rel L2 {rel:.2e}")
        assert rel <= 2e-2, (u, rel)


def test_no_request_nothing_new_and_refusals():
    from test_w8_rows_cpu import cfg
    from voicecraft_amd.engine import VoiceCraftEngine
    a, sdq, prompts = _model("tiny128")
    rows = 33
    forced = _forced(a, rows)
    eng = _engine(a, sdq, rows, w8="as_is", w8_up=False, w8_wide=True)
    assert eng.options().endswith("|w8=5|w8w=5") and "w8u" not in eng.options()
    assert all("ffn_up_wide" not in layer for layer in eng.w8_stats())
    for v in (0, 2, 10):
        with pytest.raises(AssertionError):
            eng.set_option("w8u", v)
        assert eng.options().endswith("|w8=5|w8w=5")
    c0 = eng.launch_counts()
    _multi(eng, prompts, rows, forced)
    c = _delta(eng.launch_counts(), c0)
    assert c["w8_up"] == 0 and c["w8_wide"] > 0, c
    assert eng.lib.vc_request_w8_up(eng._h, 2) == -2            # VC_ESTATE: the request comes before vc_finalize_weights
    assert eng.options().endswith("|w8=5|w8w=5")
    with pytest.raises(ValueError):
        _engine(a, sdq, rows, w8=None, w8_up=True)
    with pytest.raises(AssertionError):                         # bf16 operands: an fp32 engine refuses as it does for `w8`
        _engine(a, sdq, rows, dtype="fp32")
    for bad in (0, 1, 3, 4, 5, 10, -1):                         # not the mask 2: VC_EINVAL, an AssertionError as for every bad input
        bad_cls = type("BadMask", (VoiceCraftEngine,), {"W8_UP_MASK": bad})
        with pytest.raises(AssertionError):
            _engine(a, sdq, rows, cls=bad_cls)
    # the order of the requests, on a bare handle
    lib = eng.lib
    h = C.c_void_p()
    c_ = cfg(a.d_model, a.nhead)
    assert lib.vc_create(C.byref(c_), 0, C.byref(h)) == 0
    try:
        assert lib.vc_request_w8_up(h, 2) == -2                 # VC_ESTATE: after vc_request_w8 only
        assert lib.vc_request_w8(h, 1) == 0                     # (it needs the request, none of its bits)
        for bad in (0, 1, 4, 5, 7, 10, -1):
            assert lib.vc_request_w8_up(h, bad) == -1           # VC_EINVAL
        assert lib.vc_request_w8_wide(h, 2) == -1               # bit 2 stays no bit of the older request
        assert lib.vc_request_w8_up(h, 2) == 0
    finally:
        lib.vc_destroy(h)
    eng8 = _engine(a, sdq, rows)
    for bad in (1, 4, 5, 8, 13, 16, -1):
        with pytest.raises(AssertionError):
            eng8.set_option("w8u", bad)
        assert eng8.options().endswith("|w8=5|w8u=2")
    for bad in (2, 10):                                         # ... and bit 2 no bit of option `w8w`
        with pytest.raises(AssertionError):
            eng.set_option("w8w", bad)
    # an engine that cannot run wide steps packs nothing more
    narrow = _engine(a, sdq, 8)
    assert all(layer["ffn_up_wide"]["state"] == "not_applicable" for layer in narrow.w8_stats()), narrow.w8_stats()
