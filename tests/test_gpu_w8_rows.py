"""-m gpu: option `w8r` - on an engine created with `w8=` and `w8_rows=True`, steps of 2..8 finished rows stream the FFN
down-projection (bit 1, rows_gemm_frp_w8_k) and the QKV projection of layers 1.. (bit 4, rows_gemm_qp_w8_k) as E4M3 bytes.  The bytes
decode to the same bf16 MFMA operands and everything else is the image kernels' text (csrc/vc_gemm_frp_body.h, vc_gemm_qp_body.h), so
every result is BIT-identical to `w8r = 0`: the tests compare with np.array_equal, eager and captured, at every width with a form
(tiny128: FFN-down with 1 group per wave; giga330M: 2; giga830M: 4 and the QKV form), at both ends of both row forms (4 and 8 rows
staged), with inactive and repeated rows, through best-of-N, a decode session and a refused matrix."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_STEPS = 12
LAYERS = 2
OFF_GRID = (1.0 + 2.0 ** -7) * 2.0 ** -6          # eight significant bits: on no E4M3 grid (tests/test_gpu_w8.py)
ROWS = (2, 3, 4, 5, 6, 8)
PRESETS = ("tiny128", "giga330M", "giga830M")


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


def _has_form(preset):
    """(FFN-down, QKV of layers 1..) have a w8 form: FFN-down at every width here; QKV at d = 2048, wherever rows_gemm_qp_k runs there
    (up to 6 rows: the decode steps of a narrower call, and the last few rows of a prompt's prefill in every call)."""
    return True, preset == "giga830M"


@functools.lru_cache(maxsize=None)
def _model(preset, live=False):
    """(args, the synthetic state dict on the w8 grid, eight prompts of different shapes): computed once, never modified.
    live: terminators can be sampled (the recipe of tests/test_gpu_session.py), so that free-running calls end by themselves."""
    from voicecraft_amd import quant, synth
    a = synth.make_args(preset, num_decoder_layers=LAYERS)
    sd = synth.make_state_dict(a, seed=4, fast=True, mute_eos=False, boost=[(0, 2051, 0.45)]) if live else synth.make_state_dict(a, seed=0, fast=True)
    prompts = tuple(synth.random_prompt(a, 4 + (u % 5), 9 + 3 * (u % 7), seed=700 + u) for u in range(8))
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


def _engine(a, sd, rows, w8="as_is", w8_rows=True, dtype="bf16", cls=None, use_graph=True):
    from voicecraft_amd.engine import VoiceCraftEngine
    kw = {} if w8 is None else {"w8": w8}
    return (cls or VoiceCraftEngine)(a, sd, device="cuda:0", dtype=dtype, max_seqs=rows, max_positions=256, use_graph=use_graph,
                                     w8_rows=w8_rows, **kw)


def _multi(eng, prompts, rows, forced):
    outs, lg = eng.inference_tts_multi([p[0][0] for p in prompts[:rows]], [p[2][0] for p in prompts[:rows]], top_k=1, stop_repetition=3,
                                       _forced=forced, _logit_steps=N_STEPS)
    return [o[0].cpu().numpy() for o in outs], lg.cpu().numpy()


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("preset", PRESETS)
def test_w8r_logits_bit_identical_and_census(preset, rows):
    a, sdq, prompts = _model(preset)
    forced = _forced(a, rows)
    eng = _engine(a, sdq, rows)
    assert eng.options().endswith("|w8=5|w8r=5")
    assert all(layer["ffn_down"]["state"] == "packed" for layer in eng.w8_stats()), eng.w8_stats()
    ffn, qkv = _has_form(preset)
    for use_graph in (False, True):
        eng.use_graph = use_graph
        ref = None
        for v in (0, 1, 4, 5):
            eng.set_option("w8r", v)
            assert eng.options().endswith(f"|w8=5|w8r={v}")
            c0 = eng.launch_counts()
            res, lg = _multi(eng, prompts, rows, forced)
            c = _delta(eng.launch_counts(), c0)
            assert eng.last_steps == N_STEPS             # every row ends with the last forced step: the step width never changes
            if ref is None:
                ref = (res, lg, c)
                assert np.isfinite(lg[np.abs(lg) < 1e3]).all() and np.abs(lg).max() > 0
                assert c["w8_rows"] == 0, c
            assert np.array_equal(lg, ref[1]), (use_graph, v, float(np.abs(lg - ref[1]).max()))
            assert all(np.array_equal(r, w) for r, w in zip(res, ref[0]))
            # one FFN down-projection per layer and one paired QKV projection per layer 1.. and step (eager: every launch is counted,
            # captured: once per capture), each counted in its image twin's slot and once more in w8_rows where the plan takes the form
            frp, qp = c["rows_gemm_frp"], c["rows_gemm_qp"]
            assert frp > 0 and frp % LAYERS == 0, c
            if not use_graph:                                # (the eager loop launches steps ahead of the ones it takes)
                assert frp // LAYERS >= N_STEPS - 1, c
            if preset != "giga830M" or rows <= 6:
                assert qp == frp // LAYERS * (LAYERS - 1), c
            else:                                            # d = 2048 past 6 rows: the decode steps keep the 12-channel QKV launch,
                assert qp < frp // LAYERS * (LAYERS - 1), c  # the prompts' last few prefill rows do not
            assert c["w8_rows"] == (frp if ffn and v & 1 else 0) + (qp if qkv and v & 4 else 0), (use_graph, v, c)
            # the option moves no launch to another form.  (Captured: every launch is counted once, at capture.  The eager loop launches
            # steps ahead of the ones it takes, a number that depends on the host's timing: there only the one-row slots are compared.)
            for slot in ("rows_gemm_frp", "rows_gemm_qp", "rows_gemm_fr", "w8", "w13", "row_gemm_fr1") if use_graph else ("w8", "w13", "row_gemm_fr1"):
                assert c[slot] == ref[2][slot], (slot, v, c, ref[2])


@pytest.mark.parametrize("shrink", [1, 0])
@pytest.mark.parametrize("rows", [3, 8])
def test_w8r_inactive_and_ragged_rows(rows, shrink):
    """Row 0 ends six steps before the others: with shrink off its row stays in the step without a position, with shrink on the live
    rows move onto a narrower step where there is one (3 -> 2 rows); columns of rows a step does not have repeat its last row."""
    a, sdq, prompts = _model("giga830M")
    forced = _forced(a, rows, ends=[N_STEPS - 6] + [N_STEPS] * (rows - 1))
    eng = _engine(a, sdq, rows)
    eng.set_option("shrink", shrink)
    out = {}
    for v in (0, 5):
        eng.set_option("w8r", v)
        c0 = eng.launch_counts()
        out[v] = _multi(eng, prompts, rows, forced)
        c = _delta(eng.launch_counts(), c0)
        assert (c["w8_rows"] > 0) == bool(v), c
    (res0, lg0), (res5, lg5) = out[0], out[5]
    T = [p[2].shape[1] for p in prompts[:rows]]
    assert res0[0].shape[-1] - T[0] < res0[1].shape[-1] - T[1], [r.shape for r in res0]
    assert all(r0.shape == r5.shape and np.array_equal(r0, r5) for r0, r5 in zip(res0, res5))
    assert np.array_equal(lg0, lg5), float(np.abs(lg0 - lg5).max())


def test_w8r_best_of_three_sampled():
    a, sdq, prompts = _model("giga830M", live=True)
    x, xl, y = prompts[1]
    eng = _engine(a, sdq, 3)
    out = {}
    for v in (0, 5):
        eng.set_option("w8r", v)
        c0 = eng.launch_counts()
        res = eng.inference_tts_batch(x.cuda(), xl.cuda(), y.cuda(), top_k=40, top_p=1.0, temperature=1.0, stop_repetition=3,
                                      batch_size=3, _seed=1234)
        c = _delta(eng.launch_counts(), c0)
        assert (c["w8_rows"] > 0) == bool(v), c
        out[v] = (res[0].cpu().numpy(), list(eng.last_kept), eng.last_steps)
    assert out[0][0].shape == out[5][0].shape and np.array_equal(out[0][0], out[5][0])
    assert out[0][1:] == out[5][1:], (out[0][1:], out[5][1:])
    assert out[0][0].shape[-1] > y.shape[1]


def test_w8r_session_widths_one_to_four():
    """Six seeded requests of different lengths through four slots: the step width moves through 1..4 as requests end and join."""
    a, sdq, prompts = _model("giga830M", live=True)
    got = {}
    for v in (0, 5):
        eng = _engine(a, sdq, 4)
        eng.set_option("w8r", v)
        c0 = eng.launch_counts()
        outs = eng.inference_tts_queue([p[0][0] for p in prompts[:6]], [p[2][0] for p in prompts[:6]], max_live=4,
                                       seeds=[100 + u for u in range(6)], top_k=40, top_p=1.0, temperature=1.0, stop_repetition=3)
        c = _delta(eng.launch_counts(), c0)
        st = eng.last_session_stats
        assert st["admitted"] == 6, st
        assert c["row_gemm_fr1"] > 0 and c["rows_gemm_frp"] > 0, c          # one-row and 2..4-row steps both ran
        assert (c["w8_rows"] > 0) == bool(v) and c["w8"] > 0, c
        got[v] = [o[0].cpu().numpy() for o in outs]
        del eng
    lens = [r.shape[-1] - p[2].shape[1] for r, p in zip(got[0], prompts)]
    assert len(set(lens)) > 1, lens
    assert all(r0.shape == r5.shape and np.array_equal(r0, r5) for r0, r5 in zip(got[0], got[5]))


def test_w8r_three_rows_against_the_oracle_on_the_quantised_checkpoint():
    """Teacher-forced logits of a 3-row call meet the project's bf16 bar (per-step relative L2 <= 2e-2) against the oracle on
    the quantised checkpoint, and equal a plain bf16 engine's on that checkpoint bit for bit."""
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from test_gpu_model import rel_l2
    from voicecraft_amd import synth
    a, _, prompts = _model("tiny128")
    sd = synth.make_state_dict(a, seed=0, fast=True)
    forced = _forced(a, 3)
    eng = _engine(a, sd, 3, w8="quantize")
    c0 = eng.launch_counts()
    _, got = _multi(eng, prompts, 3, forced)
    assert _delta(eng.launch_counts(), c0)["w8_rows"] > 0
    _, plain = _multi(_engine(a, eng.w8_state_dict, 3, w8=None, w8_rows=False), prompts, 3, forced)
    assert np.array_equal(got, plain)
    torch.set_num_threads(min(4, torch.get_num_threads()))
    orc = VoiceCraftOracle(a, eng.w8_state_dict)
    for u in range(3):
        x, _, y = prompts[u]
        want = orc.tts_logits_for_trajectory(x, y, forced[:, u], steps=list(range(N_STEPS))).numpy()
        rel = float(rel_l2(got[:, u].reshape(want.shape), want).max())
        print(f"tiny128, 3 rows, utterance {u}: w8r engine against the oracle on the quantised checkpoint: worst rel L2 {rel:.2e}")
        assert rel <= 2e-2, (u, rel)


def test_w8r_one_off_grid_value_keeps_its_layer_on_the_image():
    a, sdq, prompts = _model("giga830M")
    sdq = {k: v.clone() for k, v in sdq.items()}
    sdq["decoder.layers.1.linear2.weight"][40, 200] = OFF_GRID
    rows = 3
    forced = _forced(a, rows)
    eng = _engine(a, sdq, rows, use_graph=False)
    st = eng.w8_stats()
    assert st[0]["ffn_down"]["state"] == "packed" and st[1]["ffn_down"] == {"state": "refused", "refused_fragments": 1}, st
    assert all(layer["qkv"]["state"] == "packed" for layer in st), st
    eng.set_option("w8r", 0)
    _, want = _multi(eng, prompts, rows, forced)
    # eager: every launch is counted; layer 1's FFN down-projection stays on rows_gemm_frp_k
    for v, down, qkv in ((1, LAYERS - 1, 0), (4, 0, LAYERS - 1), (5, LAYERS - 1, LAYERS - 1)):
        eng.set_option("w8r", v)
        c0 = eng.launch_counts()
        _, got = _multi(eng, prompts, rows, forced)
        c = _delta(eng.launch_counts(), c0)
        steps = c["rows_gemm_frp"] // LAYERS
        assert steps >= N_STEPS - 1 and c["rows_gemm_frp"] == steps * LAYERS and c["rows_gemm_qp"] == steps * (LAYERS - 1), c
        assert c["w8_rows"] == steps * (down + qkv), (v, c)
        assert np.array_equal(got, want), v


def test_no_request_nothing_new():
    from voicecraft_amd.engine import VoiceCraftEngine
    a, sdq, prompts = _model("tiny128")
    forced = _forced(a, 3)
    eng = _engine(a, sdq, 3, w8="quantize", w8_rows=False)
    assert eng.options().endswith("|w13=5|w8=5") and "w8r" not in eng.options()
    for v in (0, 1, 5):
        with pytest.raises(AssertionError):
            eng.set_option("w8r", v)
        assert eng.options().endswith("|w13=5|w8=5")
    c0 = eng.launch_counts()
    _multi(eng, prompts, 3, forced)
    c = _delta(eng.launch_counts(), c0)
    assert c["w8_rows"] == 0 and c["rows_gemm_frp"] > 0, c
    assert eng.lib.vc_request_w8_rows(eng._h, 5) == -2           # VC_ESTATE: the request comes before vc_finalize_weights
    with pytest.raises(ValueError):
        _engine(a, sdq, 3, w8=None, w8_rows=True)
    for w8 in ("quantize", "as_is"):                             # bf16 operands: an fp32 engine refuses as it does for `w8`
        with pytest.raises(AssertionError):
            _engine(a, sdq, 3, w8=w8, dtype="fp32")
    for bad in (2, 7, 8, -1):                                    # not a mask of 1 | 4: VC_EINVAL, an AssertionError as for every bad input
        cls = type("BadMask", (VoiceCraftEngine,), {"W8_ROWS_MASK": bad})
        with pytest.raises(AssertionError):
            _engine(a, sdq, 3, cls=cls)
    cls = type("NoSubset", (VoiceCraftEngine,), {"W8_MASK": 1})  # the rows mask must be a subset of vc_request_w8's
    with pytest.raises(AssertionError):
        _engine(a, sdq, 3, cls=cls)
    eng8 = _engine(a, sdq, 3)
    for bad in (2, 7, 8, -1):
        with pytest.raises(AssertionError):
            eng8.set_option("w8r", bad)
        assert eng8.options().endswith("|w8=5|w8r=5")
