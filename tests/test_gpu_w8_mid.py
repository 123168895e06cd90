"""-m gpu: option `w8m` - on an engine created with `w8=` and `w8_mid=True`, passes of 9..16 finished rows stream the FFN
down-projection (bit 1: rows_gemm_fr_w8_k where X fits LDS in one piece, rows_gemm_fr2_w8_k where K goes through it in two halves) as
E4M3 bytes.  The bytes decode to the same bf16 MFMA operands - one decoded fragment feeds two consecutive k-tiles - and everything else
is the image kernels' text (csrc/vc_gemm_fr_body.h, vc_gemm_fr2_body.h), so every result is BIT-identical to `w8m = 0`: the tests
compare with np.array_equal, eager and captured, at every width with a form (tiny128: one piece, 1 group per wave; giga330M: one piece,
2 groups; giga830M: two halves, 2 groups per half), at both ends of the row range, with inactive rows, through a decode session, next
to the `w8r` and `w8w` forms and with a refused matrix.  The one tolerance is the project's bf16 bar against the oracle."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_w8_mid_cpu import ROWS_WIN

pytestmark = pytest.mark.gpu

N_STEPS = 12
LAYERS = 2
OFF_GRID = (1.0 + 2.0 ** -7) * 2.0 ** -6          # eight significant bits: on no E4M3 grid (tests/test_gpu_w8.py)
ROWS = (9, 12, 16)
PRESETS = ("tiny128", "giga330M", "giga830M")
OLDER_SLOTS = ("rows_gemm_fr", "rows_gemm_frp", "rows_gemm_qp", "w8", "w8_rows", "w8_wide", "w13", "row_gemm_fr1")
ONE_ROW_SLOTS = ("w8", "w13", "row_gemm_fr1")


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


@functools.lru_cache(maxsize=None)
def _model(preset, live=False):
    """(args, the synthetic state dict on the w8 grid, 20 prompts of different shapes): computed once, never modified.
    live: terminators can be sampled (the recipe of tests/test_gpu_session.py), so that free-running calls end by themselves."""
    from voicecraft_amd import quant, synth
    a = synth.make_args(preset, num_decoder_layers=LAYERS)
    sd = synth.make_state_dict(a, seed=4, fast=True, mute_eos=False, boost=[(0, 2051, 0.45)]) if live else synth.make_state_dict(a, seed=0, fast=True)
    prompts = tuple(synth.random_prompt(a, 4 + (u % 5), 9 + 3 * (u % 7), seed=700 + u) for u in range(20))
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


def _engine(a, sd, rows, w8="as_is", w8_mid=True, dtype="bf16", cls=None, use_graph=True, **kw):
    from voicecraft_amd.engine import VoiceCraftEngine
    if w8 is not None:
        kw["w8"] = w8
    return (cls or VoiceCraftEngine)(a, sd, device="cuda:0", dtype=dtype, max_seqs=rows, max_positions=256, use_graph=use_graph,
                                     w8_mid=w8_mid, **kw)


def _multi(eng, prompts, rows, forced):
    outs, lg = eng.inference_tts_multi([p[0][0] for p in prompts[:rows]], [p[2][0] for p in prompts[:rows]], top_k=1, stop_repetition=3,
                                       _forced=forced, _logit_steps=N_STEPS)
    return [o[0].cpu().numpy() for o in outs], lg.cpu().numpy()


def _ffn_down_mid(c):
    """FFN-down launches of 9..16-row passes in a census difference.  A finished-row pass of 9..16 rows counts its out-projection and
    its FFN down-projection in rows_gemm_fr, one of 2..8 rows (the prompts' last prefill rows) its out-projection there and its FFN
    down-projection in rows_gemm_frp."""
    n2 = c["rows_gemm_fr"] - c["rows_gemm_frp"]
    assert n2 > 0 and n2 % (2 * LAYERS) == 0, c
    return n2 // 2


def _on(v, rows):
    """option value v takes the form at `rows` rows: bit 1, and bit 8 or a row count of the measured table"""
    return bool(v & 1) and (bool(v & 8) or rows in ROWS_WIN)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("preset", PRESETS)
def test_w8m_logits_bit_identical_and_census(preset, rows):
    from test_w8_rows_cpu import cfg
    a, sdq, prompts = _model(preset)
    forced = _forced(a, rows)
    eng = _engine(a, sdq, rows)
    assert eng.options().endswith("|w8=5|w8m=1")
    assert all(layer["ffn_down"]["state"] == "packed" for layer in eng.w8_stats()), eng.w8_stats()
    for use_graph in (False, True):
        eng.use_graph = use_graph
        ref = None
        for v in (0, 8, 1, 9):
            eng.set_option("w8m", v)
            assert eng.options().endswith(f"|w8=5|w8m={v}")
            plan = (C.c_int32 * 4)()
            c_ = cfg(a.d_model, a.nhead)
            assert eng.lib.vc_debug_w8m_plan(C.byref(c_), v, rows, plan) == 0 and bool(plan[0]) == _on(v, rows), (v, list(plan))
            c0 = eng.launch_counts()
            res, lg = _multi(eng, prompts, rows, forced)
            c = _delta(eng.launch_counts(), c0)
            assert eng.last_steps == N_STEPS             # every row ends with the last forced step: the step width never changes
            if ref is None:
                ref = (res, lg, c)
                assert np.isfinite(lg[np.abs(lg) < 1e3]).all() and np.abs(lg).max() > 0
            assert np.array_equal(lg, ref[1]), (use_graph, v, float(np.abs(lg - ref[1]).max()))
            assert all(np.array_equal(r, w) for r, w in zip(res, ref[0]))
            # one FFN down-projection per layer and step taken (eager: every launch is counted, and the loop launches steps ahead of the
            # ones it takes; captured: once per capture), counted in rows_gemm_fr and once more in w8_mid where the plan takes the form
            n = _ffn_down_mid(c)
            if not use_graph:
                assert n // LAYERS >= N_STEPS - 1, c
            assert c["w8_mid"] == (n if _on(v, rows) else 0), (use_graph, v, c)
            # the option moves no launch between the older slots.  (Captured: every launch is counted once, at capture.  The eager loop
            # launches steps ahead of the ones it takes, a number that depends on the host's timing: there only the one-row slots are
            # compared.)
            for slot in OLDER_SLOTS if use_graph else ONE_ROW_SLOTS:
                assert c[slot] == ref[2][slot], (slot, v, c, ref[2])


@pytest.mark.parametrize("shrink", [1, 0])
def test_w8m_inactive_and_ragged_rows(shrink):
    """Row 0 ends six steps before the others: with shrink off its row stays in the step without a position, with shrink on the live
    rows move onto an 11-row step, which still takes the form."""
    a, sdq, prompts = _model("giga830M")
    rows = 12
    forced = _forced(a, rows, ends=[N_STEPS - 6] + [N_STEPS] * (rows - 1))
    eng = _engine(a, sdq, rows)
    eng.set_option("shrink", shrink)
    out = {}
    for v in (0, 9):
        eng.set_option("w8m", v)
        c0 = eng.launch_counts()
        out[v] = _multi(eng, prompts, rows, forced)
        c = _delta(eng.launch_counts(), c0)
        assert c["w8_mid"] == (_ffn_down_mid(c) if v else 0), c
    (res0, lg0), (res9, lg9) = out[0], out[9]
    T = [p[2].shape[1] for p in prompts[:rows]]
    assert res0[0].shape[-1] - T[0] < res0[1].shape[-1] - T[1], [r.shape for r in res0]
    assert all(r0.shape == r9.shape and np.array_equal(r0, r9) for r0, r9 in zip(res0, res9))
    assert np.array_equal(lg0, lg9), float(np.abs(lg0 - lg9).max())


def test_w8m_session_widths_through_the_range():
    """18 seeded requests of different lengths through twelve slots: the step width moves through 9..12 while the queue refills the
    slots and below 9 when it drains, where the `w8r` forms take over."""
    a, sdq, prompts = _model("giga830M", live=True)
    got = {}
    for on in (False, True):
        eng = _engine(a, sdq, 12, w8_rows=True)
        assert eng.options().endswith("|w8=5|w8r=5|w8m=1")
        eng.set_option("w8m", 9 if on else 0)
        eng.set_option("w8r", 5 if on else 0)
        c0 = eng.launch_counts()
        outs = eng.inference_tts_queue([p[0][0] for p in prompts[:18]], [p[2][0] for p in prompts[:18]], max_live=12,
                                       seeds=[100 + u for u in range(18)], top_k=40, top_p=1.0, temperature=1.0, stop_repetition=3)
        c = _delta(eng.launch_counts(), c0)
        assert eng.last_session_stats["admitted"] == 18, eng.last_session_stats
        assert c["rows_gemm_fr"] > c["rows_gemm_frp"] > 0, c                # steps of 9..12 rows and of 2..8 rows both ran
        assert (c["w8_mid"] > 0) == on and (c["w8_rows"] > 0) == on, c
        got[on] = [o[0].cpu().numpy() for o in outs]
        del eng
    lens = [r.shape[-1] - p[2].shape[1] for r, p in zip(got[False], prompts)]
    assert len(set(lens)) > 1, lens
    assert all(r0.shape == r1.shape and np.array_equal(r0, r1) for r0, r1 in zip(got[False], got[True]))


def test_w8m_next_to_the_wide_form():
    """A ragged batch of 20 on an engine with `w8_wide=True` too: rows 12..19 end six steps early, the step shrinks from 20 rows (the
    pair planes) to 12 (the bytes)."""
    a, sdq, prompts = _model("giga830M")
    rows = 20
    forced = _forced(a, rows, ends=[N_STEPS - 6 if u >= 12 else N_STEPS for u in range(rows)])
    eng = _engine(a, sdq, rows, w8_wide=True)
    assert eng.options().endswith("|w8=5|w8m=1|w8w=5")
    eng.set_option("shrink", 1)
    out = {}
    for on in (False, True):
        eng.set_option("w8m", 9 if on else 0)
        eng.set_option("w8w", 13 if on else 0)
        assert eng.options().endswith("|w8=5|w8m=9|w8w=13" if on else "|w8=5|w8m=0|w8w=0")
        c0 = eng.launch_counts()
        out[on] = _multi(eng, prompts, rows, forced)
        c = _delta(eng.launch_counts(), c0)
        assert c["wd"] > 0 and c["rows_gemm_fr"] > 0, c                     # wide steps and 12-row steps both ran
        assert (c["w8_wide"] > 0) == on and (c["w8_mid"] > 0) == on, c
    (res0, lg0), (res1, lg1) = out[False], out[True]
    assert all(r0.shape == r1.shape and np.array_equal(r0, r1) for r0, r1 in zip(res0, res1))
    assert np.array_equal(lg0, lg1), float(np.abs(lg0 - lg1).max())


def test_w8m_one_off_grid_value_keeps_its_layer_on_the_image():
    a, sdq, prompts = _model("giga830M")
    sdq = {k: v.clone() for k, v in sdq.items()}
    sdq["decoder.layers.1.linear2.weight"][40, 200] = OFF_GRID
    rows = 12
    forced = _forced(a, rows)
    eng = _engine(a, sdq, rows, use_graph=False)
    st = eng.w8_stats()
    assert st[0]["ffn_down"]["state"] == "packed" and st[1]["ffn_down"] == {"state": "refused", "refused_fragments": 1}, st
    eng.set_option("w8m", 0)
    _, want = _multi(eng, prompts, rows, forced)
    eng.set_option("w8m", 9)
    c0 = eng.launch_counts()
    _, got = _multi(eng, prompts, rows, forced)
    c = _delta(eng.launch_counts(), c0)
    # eager: every launch is counted; layer 1's FFN down-projection stays on rows_gemm_fr2_k
    n = _ffn_down_mid(c)
    assert n // LAYERS >= N_STEPS - 1 and c["w8_mid"] == n // LAYERS, c
    assert np.array_equal(got, want)


def test_w8m_twelve_rows_against_the_oracle_on_the_quantised_checkpoint():
    """Teacher-forced logits of a 12-row call meet the project's bf16 bar (per-step relative L2 <= 2e-2) against the oracle on
    the quantised checkpoint for three of the rows, and equal a plain bf16 engine's on that checkpoint bit for bit."""
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from test_gpu_model import rel_l2
    from voicecraft_amd import synth
    a, _, prompts = _model("tiny128")
    sd = synth.make_state_dict(a, seed=0, fast=True)
    rows = 12
    forced = _forced(a, rows)
    eng = _engine(a, sd, rows, w8="quantize")
    eng.set_option("w8m", 9)
    c0 = eng.launch_counts()
    _, got = _multi(eng, prompts, rows, forced)
    assert _delta(eng.launch_counts(), c0)["w8_mid"] > 0
    _, plain = _multi(_engine(a, eng.w8_state_dict, rows, w8=None, w8_mid=False), prompts, rows, forced)
    assert np.array_equal(got, plain)
    torch.set_num_threads(min(4, torch.get_num_threads()))
    orc = VoiceCraftOracle(a, eng.w8_state_dict)
    for u in (0, 5, 11):
        x, _, y = prompts[u]
        want = orc.tts_logits_for_trajectory(x, y, forced[:, u], steps=list(range(N_STEPS))).numpy()
        rel = float(rel_l2(got[:, u].reshape(want.shape), want).max())
        print(f"tiny128, 12 rows, utterance {u}: w8m engine against the oracle on the quantised checkpoint: worst rel L2 {rel:.2e}")
        assert rel <= 2e-2, (u, rel)


def test_no_request_nothing_new():
    from test_w8_rows_cpu import cfg
    from voicecraft_amd.engine import VoiceCraftEngine
    a, sdq, prompts = _model("tiny128")
    rows = 12
    forced = _forced(a, rows)
    eng = _engine(a, sdq, rows, w8="quantize", w8_mid=False)
    assert eng.options().endswith("|w13=5|w8=5") and "w8m" not in eng.options()
    for v in (0, 1, 8, 9):
        with pytest.raises(AssertionError):
            eng.set_option("w8m", v)
        assert eng.options().endswith("|w13=5|w8=5")
    c0 = eng.launch_counts()
    _multi(eng, prompts, rows, forced)
    c = _delta(eng.launch_counts(), c0)
    assert c["w8_mid"] == 0 and c["rows_gemm_fr"] > 0, c
    assert eng.lib.vc_request_w8_mid(eng._h, 1) == -2           # VC_ESTATE: the request comes before vc_finalize_weights
    with pytest.raises(ValueError):
        _engine(a, sdq, rows, w8=None, w8_mid=True)
    for w8 in ("quantize", "as_is"):                            # bf16 operands: an fp32 engine refuses as it does for `w8`
        with pytest.raises(AssertionError):
            _engine(a, sdq, rows, w8=w8, dtype="fp32")
    for bad in (2, 4, 5, 8, -1):                                # not the mask 1: VC_EINVAL, an AssertionError as for every bad input
        bad_cls = type("BadMask", (VoiceCraftEngine,), {"W8_MID_MASK": bad})
        with pytest.raises(AssertionError):
            _engine(a, sdq, rows, cls=bad_cls)
    # the order of the requests, on a bare handle
    lib = eng.lib
    h = C.c_void_p()
    c_ = cfg(a.d_model, a.nhead)
    assert lib.vc_create(C.byref(c_), 0, C.byref(h)) == 0
    try:
        assert lib.vc_request_w8_mid(h, 1) == -2                # VC_ESTATE: after vc_request_w8 only
        assert lib.vc_request_w8(h, 4) == 0
        assert lib.vc_request_w8_mid(h, 1) == -1                # VC_EINVAL: no subset of the w8 request
        assert lib.vc_request_w8(h, 5) == 0
        assert lib.vc_request_w8_mid(h, 4) == -1                # VC_EINVAL: QKV has no form at 9..16 rows
        assert lib.vc_request_w8_mid(h, 5) == -1
        assert lib.vc_request_w8_mid(h, 2) == -1
        assert lib.vc_request_w8_mid(h, 1) == 0
    finally:
        lib.vc_destroy(h)
    eng8 = _engine(a, sdq, rows)
    for bad in (2, 4, 5, 16, -1):
        with pytest.raises(AssertionError):
            eng8.set_option("w8m", bad)
        assert eng8.options().endswith("|w8=5|w8m=1")
